#!/usr/bin/env python
"""Executes wrd_loss, prodwrd_loss and sumwrd_loss of the reference's own ``model/losses.py``
(:373-437) and ``get_tuple`` of its ``train/train.py`` with DISTANCE_TYPE = 'wrd' (:538-556) —
the files as they lie under /root/reference, nothing of them is copied — and freezes what they
return in tests/golden/golden_ref_wrd_v1.json.  BUILD CONTAINER ONLY: needs /root/reference.

    python tests/tools/ref_exec/make_golden_ref_wrd.py

The losses run on tests/tools/ref_exec/tf_shim.py at FLOAT64 (inputs: the float32 values of
tests/spectral_data.py, widened).  tf_shim refuses ``tf.linalg.svd`` and ``tf.slice`` and has no
``tf.reduce_prod``; this file — not the shim — supplies NumPy stand-ins for the three:
``np.linalg.svd(x, compute_uv=False)`` (descending, like TensorFlow's), plain slicing with
``size = -1`` meaning "to the end", and ``np.prod``.  The slice stand-in records what it returns:
the ``dimensions`` largest singular values of the positive and of the negative side, whose
products the golden file keeps beside the loss (the loss alone is the margin plus a difference
of products of 1e-5 and smaller).
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_trainer import ROOT, install_names, load_trainer  # noqa: E402
import tf_shim  # noqa: E402
from make_golden_ref import load_reference  # noqa: E402
from tests import spectral_data as D  # noqa: E402
from tests import util_data as U  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'golden_ref_wrd_v1.json')
SLICES = []


def _svd(tensor, full_matrices=False, compute_uv=True, name=None):
    assert not compute_uv
    tf_shim._count('linalg.svd')
    return tf_shim._t(np.linalg.svd(tf_shim._t(tensor).view(np.ndarray), compute_uv=False))


def _slice(input_, begin, size, name=None):
    tf_shim._count('slice')
    a = tf_shim._t(input_).view(np.ndarray)
    idx = tuple(slice(int(b), None if int(s) == -1 else int(b) + int(s)) for b, s in zip(begin, size))
    out = a[idx]
    SLICES.append(np.array(out, dtype=np.float64))
    return tf_shim._t(out)


def install_stand_ins():
    tf_shim.linalg.svd = _svd
    tf_shim.slice = _slice
    tf_shim.reduce_prod = tf_shim._reduce('reduce_prod', np.prod)


LOSS_CASES = [   # (T, P, N, E, dimensions, seed); dimensions <= min(P, N) - 1
    (2, 4, 4, 64, 3, 11),
    (3, 5, 7, 200, 4, 12),
    (2, 12, 12, 512, 10, 13),
]


def main():
    install_stand_ins()
    R = load_reference()
    f64 = np.float64
    losses = []
    for kind in ('wrd', 'prodwrd', 'sumwrd'):
        fn = getattr(R, kind + '_loss')
        for t, p, n, e, k, seed in LOSS_CASES:
            z, pw, nw = D.tuples(t, p, n, e, seed)
            z = z.astype(f64)
            del SLICES[:]
            val = fn(tf_shim._t(z[:, :1]), tf_shim._t(z[:, 1:1 + p]), tf_shim._t(z[:, 1 + p:]),
                     tf_shim._t(pw.astype(f64)[:, :, None]), tf_shim._t(nw.astype(f64)[:, :, None]),
                     0.1, dimensions=k)
            assert len(SLICES) == 2 and np.asarray(val).dtype == f64
            prods = np.stack([SLICES[0].prod(1), SLICES[1].prod(1)], 1)
            losses.append({'kind': kind, 't': t, 'p': p, 'n': n, 'e': e, 'dimensions': k, 'seed': seed,
                           'margin': 0.1, 'loss': float(val), 'prods': prods.tolist()})
            print('%-8s T%d P%d N%d E%d k%d loss %.12g' % (kind, t, p, n, e, k, float(val)))

    from sklearn.neighbors import KDTree
    import threading
    install_names()
    T = load_trainer()
    T.LOG = open(os.devnull, 'w')
    xy, yaw = U.sampler_dataset()
    num = len(yaw)
    meta = {'date': ['d'] * num, 'folder': ['1'] * num, 't': [str(i) for i in range(num)]}
    tree = KDTree(xy)
    samples = []
    for name, shape, anchors, seed, alpha, beta in (
            ('wrd_tu1_p12_n12', [1, 12, 12], [77], 21, 0.8, 15),
            ('wrd_tu3_p4_n6', [1, 4, 6], [0, 150, 301], 22, 0.8, 15),
            ('wrd_tu2_p3_n5_other_alpha_beta', [1, 3, 5], [33, 250], 23, 0.5, 20.0)):
        g = dict(POSITIVES_PER_TUPLE=shape[1], NEGATIVES_PER_TUPLE=shape[2], MAX_POS_RADIUS=15.0,
                 MIN_NEG_RADIUS=15.0, HARD_POSITIVES_PER_TUPLE=6, HARD_NEGATIVES_PER_TUPLE=6,
                 MUTUALLY_EXCLUSIVE_NEGS=True, MINING_CACHE_SIZE=1000, ALPHA=alpha, BETA=beta)
        for key, v in g.items():
            setattr(T, key, v)
        T.DISTANCE_TYPE = 'wrd'
        T.CACHED_FEATURE_LOCK = threading.Lock()
        np.random.seed(seed)
        distances, image_info, _last = T.get_tuple(anchors, shape, False, meta, xy, yaw, tree)
        samples.append({'name': name, 'tuple_shape': shape, 'anchors': anchors, 'seed': seed,
                        'alpha': alpha, 'beta': beta,
                        'indices': [int(info[2]) for info in image_info],
                        'distances': [np.asarray(d, dtype=np.float64).tolist() for d in distances]})
        print('%-34s %3d images, payload %d x %d' % (name, len(image_info), len(distances),
                                                     len(distances[0])))
    import sklearn
    meta_out = {'made_by': 'tests/tools/ref_exec/make_golden_ref_wrd.py',
                'what': "wrd_loss / prodwrd_loss / sumwrd_loss of /root/reference/model/losses.py at float64 on "
                        "tests/tools/ref_exec/tf_shim.py with NumPy stand-ins for tf.linalg.svd, tf.slice and "
                        "tf.reduce_prod (inputs: tests/spectral_data.tuples); get_tuple() of "
                        "/root/reference/train/train.py with DISTANCE_TYPE = 'wrd' on "
                        "tests/util_data.sampler_dataset (np.random.seed(seed) before each call)",
                'numpy': np.__version__, 'sklearn': sklearn.__version__}
    with open(OUT, 'w') as f:
        json.dump({'meta': meta_out, 'losses': losses, 'sampler': samples}, f, indent=1)
    print('wrote %s' % OUT)


if __name__ == '__main__':
    main()

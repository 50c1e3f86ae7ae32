"""Seeded inputs of the wrd / prodwrd / sumwrd tests (and of the generator of their golden file,
tests/tools/ref_exec/make_golden_ref_wrd.py): descriptors clustered like a trained embedder's and
the trainer's 'wrd' payload.

Rows are ``c + 0.3 u`` with a unit vector ``c`` common to the tuple and a unit Gaussian direction
``u`` per row, L2-normalised, float32.  Positives lie 0.5..15 m from the anchor, negatives
15..80 m; the weights are the sampler's ``1/(1+e^(alpha(d-beta)))`` and
``1/(1+e^(alpha(beta-d)))`` with alpha = 0.8, beta = 15, float32 like the trainer's placeholder.
On 300 draws per shape this gives s_k / s_1 >= 0.18 and (s_k - s_{k+1}) / s_1 >= 3e-5 for
k <= min(P, N) - 1 (the tests assert looser bounds on their own draws); with more singular values
than well-weighted rows the k-th one is 1e-9 .. 1e-15 of the first and the product is noise.
"""
import numpy as np

ALPHA, BETA = 0.8, 15.0


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def tuples(t, p, n, e, seed):
    """-> z [T, 1+P+N, E] float32 (row 0 the anchor), pos_w, neg_w [T, P+N] float32."""
    rng = np.random.RandomState(seed)
    c = _unit(rng.randn(t, 1, e))
    u = _unit(rng.randn(t, 1 + p + n, e))
    z = _unit(c + 0.3 * u).astype(np.float32)
    d = np.concatenate([rng.uniform(0.5, 15.0, (t, p)), rng.uniform(15.0, 80.0, (t, n))], 1)
    pos_w = (1.0 / (1.0 + np.exp(ALPHA * (d - BETA)))).astype(np.float32)
    neg_w = (1.0 / (1.0 + np.exp(ALPHA * (BETA - d)))).astype(np.float32)
    return z, pos_w, neg_w

"""Inputs shared by tests/test_vlad_init_host.py and tests/test_gpu_vlad_init.py: the two real-valued
descriptor sets of the k-means tests and the seeded centres."""
import numpy as np

N, K, D = 4096, 64, 512


def _unit(x):
    return (x / np.sqrt((x * x).sum(axis=1, keepdims=True))).astype(np.float32)


def gauss(n=N):
    """Isotropic rows on the sphere: no cluster structure, many near-ties."""
    return _unit(np.random.RandomState(0).randn(n, D))


def mix(n=N):
    """64 blobs on the sphere with noise of 1.5 per coordinate around means of unit variance."""
    rng = np.random.RandomState(0)
    m = rng.randn(64, D)
    return _unit(m[rng.randint(0, 64, n)] + 1.5 * rng.randn(n, D))


def seeds(x, k=K, seed=0):
    """The rows kmeans() starts from."""
    return x[np.random.RandomState(seed).permutation(len(x))[:k]].copy()


def integers(n, k, seed):
    """x [n, 512] and centres [k, 512] of integers in [-4, 4] as float32, offsets |c|^2 / 2: every
    score, sum and inertia is exact in float32 resp. float64."""
    rng = np.random.RandomState(seed)
    x = rng.randint(-4, 5, (n, D)).astype(np.float32)
    c = rng.randint(-4, 5, (k, D)).astype(np.float32)
    if k > 2:
        c[k - 1] = c[0]                                  # a twin: it loses every tie
    if n > 2:
        x[n - 1] = x[0]
    off = (0.5 * (c.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    return x, c, off

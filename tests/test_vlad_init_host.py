"""Host-side checks of the NetVLAD head from data (no GPU): the C-ABI additions of include/scl_hip.h
(declared, exported, bound, the size query, validation before any launch), the NumPy statement of a
Lloyd step and of the head construction in model/vlad_init.py, and the trainer's new flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import vlad_init_data as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scl_hip.h")
NEW = ("scl_kmeans_workspace_bytes", "scl_kmeans_assign", "scl_kmeans_update")
NULL, SHAPE, WORKSPACE = -3, -1, -4


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from soft_contrastive_learning_amd import _lib
    return _lib.load()


# ---- the C ABI ------------------------------------------------------------------------------------

def test_the_three_symbols_are_declared_exported_and_bound(lib):
    from soft_contrastive_learning_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(scl_[a-z0-9_]+)\s*\(", src))
    diag = _lib.load(diag=True)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None and getattr(diag, name) is not None
    assert re.search(r"#define\s+SCL_ABI_VERSION\s+12\b", src)          # purely additive
    assert re.search(r"#define\s+SCL_KMEANS_ROWS\s+%d\b" % _lib.KMEANS_ROWS, src)
    assert re.search(r"#define\s+SCL_KMEANS_MAX_N\s+\(1 << 22\)", src) and _lib.KMEANS_MAX_N == 1 << 22


def test_workspace_query_is_a_pure_host_function(lib):
    from soft_contrastive_learning_amd import _lib
    f = lib.scl_kmeans_workspace_bytes
    assert f(100, 0) == 0 and f(100, 65) == 0 and f(0, 64) == 0 and f(-5, 64) == 0 and f(100, -1) == 0
    assert f(_lib.KMEANS_MAX_N + 1, 64) == 0
    for n in (1, 127, 128, 129, 50000, _lib.KMEANS_MAX_N):
        for k in (1, 3, 64):
            got = f(n, k)
            assert got > 0 and got % 256 == 0
            assert got >= 64 * 512 * 4 + 64 * 4           # the operand image of the centres and its offsets


def test_validation_happens_before_any_launch_in_the_order_null_shape_workspace(lib):
    """Every refusal is asserted with a condition that a LATER check refuses also present."""
    buf = ctypes.create_string_buffer(1 << 18)
    base = (ctypes.addressof(buf) + 255) & ~255
    p, a4, a16 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 16)
    ws = lib.scl_kmeans_workspace_bytes(200, 64)

    def assign(x=p, n=200, c=p, off=p, k=64, label=p, best=p, second=p, psum=None, pcnt=None, pin=None,
               work=p, nbytes=ws):
        return lib.scl_kmeans_assign(x, n, c, off, k, label, best, second, psum, pcnt, pin, work, nbytes, None)

    # NULL — with a bad shape (K = 65) and no workspace bytes also present
    for kw in (dict(x=None), dict(c=None), dict(off=None), dict(label=None), dict(best=None),
               dict(second=None), dict(work=None)):
        assert assign(k=65, nbytes=0, **kw) == NULL, kw
    assert assign(psum=p, pcnt=None, pin=p, k=65, nbytes=0) == NULL       # sums without their counts
    assert assign(psum=p, pcnt=p, pin=None, n=0, nbytes=0) == NULL        # ... without their inertia
    # shape — with a workspace that is too small also present
    for kw in (dict(n=0), dict(n=-1), dict(n=(1 << 22) + 1), dict(k=0), dict(k=65), dict(x=a4), dict(c=a4),
               dict(psum=a4, pcnt=p, pin=p)):
        assert assign(nbytes=0, **kw) == SHAPE, kw
    # workspace: one byte short, not 256-byte aligned
    assert assign(nbytes=ws - 1) == WORKSPACE and assign(work=a16) == WORKSPACE
    assert assign(psum=p, pcnt=p, pin=p, nbytes=ws - 1) == WORKSPACE

    def update(psum=p, pcnt=p, pin=p, g=2, k=64, old=p, new=a16, counts=p, inertia=p):
        return lib.scl_kmeans_update(psum, pcnt, pin, g, k, old, new, counts, inertia, None)

    for kw in (dict(psum=None), dict(pcnt=None), dict(pin=None), dict(old=None), dict(new=None),
               dict(counts=None), dict(inertia=None)):
        assert update(k=65, **kw) == NULL, kw
    for kw in (dict(g=0), dict(g=(1 << 22) // 128 + 1), dict(k=0), dict(k=65), dict(psum=a4), dict(old=a4),
               dict(new=a4), dict(new=p)):                                 # new == old: no update in place
        assert update(**kw) == SHAPE, kw


# ---- the NumPy statement ----------------------------------------------------------------------------

def test_assign_np_ties_nan_and_a_single_cluster():
    from soft_contrastive_learning_amd.model import vlad_init as VI
    c = np.zeros((4, 512), dtype=np.float32)
    c[0, 0], c[1, 0], c[2, 1], c[3, 2] = 1.0, 1.0, 1.0, np.nan            # 0 and 1 are twins; 3 scores NaN
    x = np.zeros((4, 512), dtype=np.float32)
    x[0, 0] = 2.0                      # scores 2, 2, 0, NaN: the tie goes to the lowest k
    x[1, 1] = 3.0                      # scores 0, 0, 3, NaN
    x[2, :] = np.nan                   # every score NaN: nothing wins
    x[3, 0] = np.inf                   # +inf, +inf, NaN (inf * 0), NaN: +inf wins, lowest k
    label, best, second = VI.assign_np(x, c, np.zeros(4, dtype=np.float32))
    assert label.dtype == np.int32 and label.tolist() == [0, 2, -1, 0]
    assert best.tolist()[:2] == [2.0, 3.0] and best[2] == -np.inf and best[3] == np.inf
    assert second.tolist()[:2] == [2.0, 0.0] and second[2] == -np.inf and second[3] == np.inf
    # a NaN score never wins, whatever the others are; -inf (an infinite offset) never does either
    label, best, second = VI.assign_np(x[:2], c, np.array([0.0, np.inf, 5.0, 0.0], dtype=np.float32))
    assert label.tolist() == [0, 0] and best.tolist() == [2.0, 0.0] and second.tolist() == [-5.0, -2.0]
    label, best, second = VI.assign_np(x[:2], c[:1], np.zeros(1, dtype=np.float32))
    assert label.tolist() == [0, 0] and (second == -np.inf).all()         # K = 1


def test_kmeans_step_np_keeps_the_centre_of_an_empty_cluster():
    from soft_contrastive_learning_amd.model import vlad_init as VI
    x = V.mix(256)
    c = V.seeds(x, 8)
    c[5] = c[2]                                                            # the twin gets no row
    new, labels, counts, inertia = VI.kmeans_step_np(x, c)
    assert counts[5] == 0 and counts.sum() == 256 and (labels != 5).all()
    np.testing.assert_array_equal(new[5], c[5])
    for k in (0, 2, 7):
        np.testing.assert_array_equal(new[k], x[labels == k].astype(np.float64).mean(axis=0).astype(np.float32))
    d2 = ((x.astype(np.float64)[:, None] - c.astype(np.float64)[None]) ** 2).sum(axis=2).min(axis=1).sum()
    assert abs(inertia - d2) <= 1e-6 * d2             # |x|^2 - 2 best is the squared distance (offsets are float32)


def test_inertia_does_not_rise_over_ten_steps_on_mix():
    from soft_contrastive_learning_amd.model import vlad_init as VI
    x = V.mix()
    c = V.seeds(x)
    seen = []
    for _ in range(10):
        c, _, _, inertia = VI.kmeans_step_np(x, c)
        seen.append(inertia)
    # each step's centres are rounded to float32 (and its offsets once more): a relative 2^-22 of slack
    assert all(b <= a * (1 + 2.0 ** -22) for a, b in zip(seen, seen[1:])), seen
    assert seen[-1] < 0.9 * seen[0]


def test_head_from_centres_arithmetic():
    from soft_contrastive_learning_amd.model import vlad_init as VI
    x = V.mix(1024)
    c, _, _, _ = VI.kmeans_step_np(x, V.seeds(x, 16))
    kernel, centers, alpha = VI.head_from_centres_np(c, x)
    assert kernel.shape == (1, 1, 512, 16) and centers.shape == (1, 1, 1, 512, 16)
    assert kernel.dtype == np.float32 and centers.dtype == np.float32
    unit = (c.astype(np.float64) / np.sqrt((c.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(np.float32)
    _, best, second = VI.assign_np(x, unit, np.zeros(16))
    mean_gap = (best - second).mean()
    assert abs(math.exp(-alpha * mean_gap) - 0.01) <= 1e-12
    np.testing.assert_array_equal(centers[0, 0, 0].T, -c)
    norms = np.sqrt((kernel[0, 0].astype(np.float64) ** 2).sum(axis=0))
    np.testing.assert_allclose(norms, alpha, rtol=3e-7)                   # float32 columns of alpha c/|c|
    with pytest.raises(ValueError):
        VI.head_from_centres_np(c[:1], x)                                  # K < 2
    bad = c.copy()
    bad[3] = 0.0
    with pytest.raises(ValueError):
        VI.head_from_centres_np(bad, x)                                    # a centre of zero norm
    with pytest.raises(ValueError):
        VI.head_from_centres_np(np.stack([c[0], c[0]]), x)                 # twins: the gap is zero everywhere


# ---- the trainer's flags -----------------------------------------------------------------------------

def test_trainer_refuses_vlad_init_kmeans_without_what_it_needs():
    from soft_contrastive_learning_amd.train import train
    flags = train.make_parser().parse_args([])
    assert flags.vlad_init == 'none' and flags.vlad_init_images == 500 and flags.vlad_init_per_image == 100
    assert flags.vlad_init_iters == 100 and flags.vlad_init_seed == 0
    ok = ['--vlad_init', 'kmeans', '--synthetic_dataset', '40']
    train.check_vlad_init(train.make_parser().parse_args(ok))
    train.check_vlad_init(train.make_parser().parse_args(['--vlad_init', 'kmeans', '--shuffled_root', 'lists']))
    for extra, word in ((['--resume'], '--resume'), (['--vlad_cores', '0'], '--vlad_cores 64')):
        with pytest.raises(SystemExit, match=word):
            train.main(ok + extra)                                         # refused before any device is touched
    with pytest.raises(SystemExit, match='--synthetic_dataset'):
        train.main(['--vlad_init', 'kmeans'])
    with pytest.raises(SystemExit):
        train.make_parser().parse_args(['--vlad_init', 'kmeanspp'])

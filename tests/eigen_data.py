"""Shared by the eigenvalue / residual loss tests (tests/test_gpu_eigen_loss.py) and the generator
of their golden file (tests/tools/ref_exec/make_golden_ref_eigen.py): a literal float64
restatement of the reference (model/losses.py:310-370, 613-624) on torch-CPU ``svdvals`` /
``eigvalsh`` autograd, the well-posedness conditions a case must meet on its ORACLE, and the
input tweaks of the hinge losses.  Inputs are tests/spectral_data.tuples.
"""
import numpy as np
import torch

RESIDUAL = ('residual_det', 'residual_trace', 'swrd')
HINGE = ('ntuplet_evmm', 'ntuplet_trace')
KINDS = RESIDUAL + HINGE + ('neg_eigenvalue',)


def reference_f64(kind, z, p, margin, k=None, pos_w=None, neg_w=None):
    """-> loss, terms [T,2], d loss / d z, (spectrum_pos, spectrum_neg).

    ``z`` [T,1+P+N,E]; ``pos_w`` [T,P] / ``neg_w`` [T,N] for swrd.  The spectra are the singular
    values (descending) of the residual kinds and the eigenvalues (ascending) of the Gram kinds;
    None where the kind takes none.  neg_eigenvalue ignores the positive rows (zero gradient)."""
    z = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    a, pos, neg = z[:, :1], z[:, 1:1 + p], z[:, 1 + p:]
    zero = torch.zeros(z.shape[0], dtype=torch.float64)
    if kind in RESIDUAL:
        yp, yn = pos - a, neg - a
        if kind == 'swrd':
            yp = yp * torch.tensor(np.asarray(pos_w, dtype=np.float64))[:, :, None]
            yn = yn * torch.tensor(np.asarray(neg_w, dtype=np.float64))[:, :, None]
        sp, sn = torch.linalg.svdvals(yp), torch.linalg.svdvals(yn)
        if kind == 'residual_trace':
            tp, tn = sp[:, :k].sum(1), sn[:, :k].sum(1)
        else:
            tp, tn = sp[:, :k].prod(1), sn[:, :k].prod(1)
        loss = (tp - tn + margin).mean(0)
    else:
        fp, fn = torch.cat([a, pos], 1), torch.cat([a, neg], 1)
        gp, gn = fp @ fp.transpose(1, 2), fn @ fn.transpose(1, 2)
        sp, sn = torch.linalg.eigvalsh(gp), torch.linalg.eigvalsh(gn)
        if kind == 'ntuplet_evmm':
            tp, tn = sp[:, 0], sn[:, -1]
        elif kind == 'ntuplet_trace':
            tp, tn = gp.diagonal(dim1=1, dim2=2).sum(1), gn.diagonal(dim1=1, dim2=2).sum(1)
            sp = sn = None
        else:
            tp, tn, sp = zero, sn[:, 0], None
        if kind == 'neg_eigenvalue':
            loss = -tn.mean(0)
        else:
            loss = torch.maximum(margin + tp - tn, zero).mean(0)
    loss.backward()
    spectra = tuple(None if s is None else s.detach().numpy() for s in (sp, sn))
    return (float(loss.detach()), torch.stack([tp, tn], 1).detach().numpy(), z.grad.numpy(), spectra)


def assert_singular_values_well_posed(sv, k):
    """[.., n] descending: the k-th is not noise and, below the row count, apart from the next."""
    s1, sk = sv[..., 0], sv[..., k - 1]
    assert (sk / s1).min() >= 0.05, (sk / s1).min()
    if sv.shape[-1] > k:
        assert ((sk - sv[..., k]) / s1).min() >= 1e-5, ((sk - sv[..., k]) / s1).min()


def assert_eigenvalue_well_posed(eig, largest):
    """[.., n] ascending: the chosen extreme eigenvalue is apart from its neighbour."""
    gap = eig[..., -1] - eig[..., -2] if largest else eig[..., 1] - eig[..., 0]
    assert (gap / eig[..., -1]).min() >= 1e-5, (gap / eig[..., -1]).min()


def assert_well_posed(kind, spectra, k):
    sp, sn = spectra
    if kind in RESIDUAL:
        assert_singular_values_well_posed(sp, k)
        assert_singular_values_well_posed(sn, k)
    elif kind == 'ntuplet_evmm':
        assert_eigenvalue_well_posed(sp, largest=False)
        assert_eigenvalue_well_posed(sn, largest=True)
    elif kind == 'neg_eigenvalue':
        assert_eigenvalue_well_posed(sn, largest=False)


def hinge_margin(raw):
    """The float32 nearest to minus the midpoint of the two middle raw hinge arguments
    ``term_pos - term_neg`` (T >= 2): one of the two is then active and the other inactive.  The
    C ABI carries the margin as float32, so the oracle must use this very value."""
    a = np.sort(np.asarray(raw, dtype=np.float64))
    return float(np.float32(-0.5 * (a[len(a) // 2 - 1] + a[len(a) // 2])))


def scale_rows(z, seed):
    """ntuplet_trace: unit rows make both traces constants (1 + P and 1 + N), so every row is
    scaled by its own factor in [0.5, 1.5]; float32 like ``z``."""
    f = np.random.RandomState(seed).uniform(0.5, 1.5, size=z.shape[:2] + (1,))
    return (z * f).astype(np.float32)

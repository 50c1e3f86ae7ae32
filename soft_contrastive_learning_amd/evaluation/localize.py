"""Frame in, position out: localisation of single frames against a resident reference index.

``evaluation/top_n.py`` answers whole query sets in one call, like the reference's
``evaluation/top-n.py``.  A trained localiser is used the other way round: the reference database
is fixed, frames arrive one or a few at a time, and each wants its position.  ``Localizer`` thins
the references (``top_n.thin_reference``, evaluation/top-n.py:91-94), whitens them row by row
(``PCAWhitening.transform_rows``: a frame's bits do not depend on its batch), prepares them once
(``retrieval.RetrievalIndex``) and then answers every call with one streaming pass of
csrc/topn.hip over the index.  The lists are the certified exact ones of ``retrieval.topn_l2``.

A tracking caller knows roughly where the vehicle is: ``near`` / ``radius`` restrict a call to the
references within ``radius`` metres of ``near`` (``RetrievalIndex.query``'s window: still the exact
top-n, of those references), so a look-alike place elsewhere on the map cannot match and the pass
over the index costs what the window covers.

The command feeds a query set through a ``Localizer`` ``--batch`` frames at a time and writes the
pickle ``top_n.main`` writes (evaluation/top-n.py:119), so the two can be compared file by file.
"""
import numpy as np
import torch

from . import retrieval
from .top_n import out_pickle_path, thin_reference


class Localizer:
    """``Localizer(ref_desc, ref_xy, pca=None, model=None, n=5, l=0.0, score='f32', device='cuda')``

    ref_desc [M, E] descriptors of the reference frames (``evaluation/inference.py``'s pickle),
    ref_xy [M, 2] their positions, ``pca`` a fitted ``PCAWhitening`` (None: the descriptors are
    used as they are), ``model`` the network of ``locate`` (None: ``nets.default_model()``), ``n``
    hits per frame, ``l`` the thinning distance in metres.

    ``query_fn(ref_f, query_f, n) -> (dist [Q,n], idx [Q,n])`` on NumPy arrays replaces the index
    in the CPU tests of the bookkeeping around it (a window is applied there by subsetting the
    rows on the host); the product path has no such argument and no CPU fallback.

    ``wide`` is ``RetrievalIndex``'s: with more than 256 (whitened) columns, 'resident' (it needs
    ``score='f32'``) keeps the frame-at-a-time route and the window; 'delegate', the default, answers
    every call with ``topn_l2`` and takes no window."""

    def __init__(self, ref_desc, ref_xy, pca=None, model=None, n=5, l=0.0, score='f32', device='cuda',
                 query_fn=None, wide='delegate'):
        self.ref_xy = np.asarray(ref_xy, dtype=np.float64)
        self.ref_idx = thin_reference(self.ref_xy, l)
        self.n = int(n)
        if len(self.ref_idx) < self.n:
            raise ValueError('%d references survive the thinning at l=%g, fewer than n=%d'
                             % (len(self.ref_idx), l, self.n))
        self._orig = np.asarray(self.ref_idx, dtype=np.int64)       # thinned row -> original index
        self.pca = pca
        self.model = model
        self._query_fn = query_fn
        self.uncertified = 0                                          # over all calls so far
        self._resizer = None                                          # prepare_raw's, made on first use
        rows = np.asarray(ref_desc, dtype=np.float32)[self._orig]
        if query_fn is not None:
            self.device = None
            self._ref_f = self._whiten(rows)
            self._index = None
            return
        self.device = torch.device(device)
        self._index = retrieval.RetrievalIndex(self._whiten(rows), 0, score,
                                               positions=self.ref_xy[self._orig], wide=wide)

    def _whiten(self, rows):
        """[m, E] NumPy or tensor -> what the index holds: device float32 rows (NumPy with query_fn)."""
        if self.pca is not None:
            rows = self.pca.transform_rows(rows)
        if self._query_fn is not None:
            return rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows, np.float32)
        t = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows))
        return t.to(self.device, torch.float32).contiguous()

    def query_thinned(self, desc, near=None, radius=None):
        """desc [Q, E] -> (feature_dist [Q, n] float64, rows of the THINNED list [Q, n] int64), NumPy.
        ``near`` [Q, 2] (or one [2] for all) and ``radius`` (a scalar or [Q]), in the units of ref_xy:
        only references within ``radius`` of ``near`` are searched; a frame with fewer than n of
        them gets row -1 and distance inf in the columns that are left."""
        f = self._whiten(desc if isinstance(desc, torch.Tensor) else np.asarray(desc, dtype=np.float32))
        if near is None and radius is None:
            if self._query_fn is not None:
                dist, idx = self._query_fn(self._ref_f, f, self.n)
                return np.asarray(dist, dtype=np.float64), np.asarray(idx, dtype=np.int64)
            stats = {}
            dist, idx = self._index.query(f, self.n, stats=stats)
            self.uncertified += stats.get('uncertified') or 0
            return dist.cpu().numpy(), idx.cpu().numpy()
        if near is None or radius is None:
            raise ValueError('a window needs both near and radius')
        q = len(f)
        near = np.array(np.broadcast_to(np.asarray(near, dtype=np.float64), (q, 2)))
        radius = np.array(np.broadcast_to(np.asarray(radius, dtype=np.float64), (q,)))
        if self._query_fn is None:
            stats = {}
            dist, idx = self._index.query(f, self.n, stats=stats, near=near, radius=radius)
            self.uncertified += stats.get('uncertified') or 0
            return dist.cpu().numpy(), idx.cpu().numpy()
        xy = self.ref_xy[self._orig]
        dist = np.full((q, self.n), np.inf, dtype=np.float64)
        idx = np.full((q, self.n), -1, dtype=np.int64)
        for k in range(q):
            dx, dy = xy[:, 0] - near[k, 0], xy[:, 1] - near[k, 1]
            member = np.nonzero((radius[k] >= 0) & (dx * dx + dy * dy <= radius[k] * radius[k]))[0]
            m = min(self.n, len(member))
            if m:
                dd, ii = self._query_fn(self._ref_f[member], f[k:k + 1], m)
                dist[k, :m], idx[k, :m] = np.asarray(dd)[0], member[np.asarray(ii)[0]]
        return dist, idx

    def locate_descriptors(self, desc, near=None, radius=None):
        """desc [Q, E] -> (idx [Q, n] original reference indices, feature_dist [Q, n] float64,
        xy [Q, n, 2]); ``xy[:, 0]`` is the position estimate.  With ``near`` / ``radius`` (see
        ``query_thinned``) a missing hit is index -1, distance inf and position NaN."""
        dist, local = self.query_thinned(desc, near, radius)
        found = local >= 0
        idx = np.where(found, self._orig[np.where(found, local, 0)], -1)
        xy = np.where(found[..., None], self.ref_xy[np.where(found, idx, 0)], np.nan)
        return idx, dist, xy

    def locate(self, images, near=None, radius=None):
        """images [B, H, W, {1|3}] raw 0..255 -> ``locate_descriptors`` of ``nets.output``."""
        from ..model import nets
        model = self.model or nets.default_model()
        with torch.no_grad():
            t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
            desc = nets.output(t.to(next(model.parameters()).device), model=model).float()
        return self.locate_descriptors(desc, near, radius)

    def prepare_raw(self, frames, rule='resize_img', bayer=None, lut=None, border='reflect', **kw):
        """Frames as the camera or the decoder delivers them (uint8 [SH,SW,C] or [n,SH,SW,C],
        NumPy or tensor, host or device) -> the float32 device batch the network sees, sized on the
        device by the loaders' rule (util/device_cv.py; bit for bit the host's util/cv.py):
        ``'resize_img'`` (``max_size=240``), ``'standard_size'`` (``h=180, w=240``) or ``'none'``
        (widened only).

        ``bayer`` (a pattern of ``util/robotcar.py``: 'gbrg' for the RobotCar stereo cameras): the
        frames are raw one-channel Bayer mosaics, [SH,SW] or [n,SH,SW]; they are demosaiced,
        undistorted by the camera's table ``lut`` (``robotcar.load_distortion_lut``; None: not at all)
        and sized in one launch (``DeviceResizer.debayer``: ``robotcar.load_image_np`` then the rule,
        bit for bit).  ``bayer=None``: ``lut`` and ``border`` are not read."""
        from ..util.device_cv import DeviceResizer
        if self._resizer is None:
            model = self.model
            device = self.device if model is None else next(model.parameters()).device
            self._resizer = DeviceResizer('cpu' if device is None else device)   # a CPU device raises
        if bayer is not None:
            return self._resizer.debayer(frames, bayer, lut, border, rule, torch.float32, **kw)
        return self._resizer.apply(frames, rule, torch.float32, **kw)

    def locate_raw(self, frames, rule='resize_img', near=None, radius=None, bayer=None, lut=None,
                   border='reflect', **kw):
        """``locate`` of ``prepare_raw(frames, rule, bayer, lut, border, **kw)``."""
        return self.locate(self.prepare_raw(frames, rule, bayer, lut, border, **kw), near, radius)

    def explain(self, images, k=0, mode='gradcam', near=None, radius=None):
        """``locate(images, near, radius)`` plus WHY: -> (idx, feature_dist, xy, map [B, h, w] float32,
        scale [B] float32), the last two on the device (evaluation/saliency.py: ``MatchSaliency.explain``;
        draw them with ``saliency.overlay``).  Each frame is explained against the index's own
        whitened row of its k-th hit; a frame without a k-th hit (row -1 under a window) gets an
        all-zero map and scale 0.  Needs the resident index: with ``query_fn`` it raises."""
        if self._index is None:
            raise ValueError('explain needs the resident index and the device model: a Localizer made '
                             'with query_fn has neither')
        from ..model import nets
        from .saliency import MatchSaliency
        k = int(k)
        if not 0 <= k < self.n:
            raise ValueError('k=%d: the localiser keeps n=%d hits per frame' % (k, self.n))
        model = self.model or nets.default_model()
        with torch.no_grad():
            t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
            t = t.to(next(model.parameters()).device)
            desc = nets.output(t, model=model).float()
        dist, local = self.query_thinned(desc, near, radius)
        found = local >= 0
        idx = np.where(found, self._orig[np.where(found, local, 0)], -1)
        xy = np.where(found[..., None], self.ref_xy[np.where(found, idx, 0)], np.nan)
        rows = torch.from_numpy(np.where(found[:, k], local[:, k], 0)).to(self._index.ref.device)
        target = self._index.ref[rows, :self._index.width]
        m, scale = MatchSaliency(model, self.pca).explain(t, target, mode)
        hit = torch.from_numpy(found[:, k]).to(m.device)
        return (idx, dist, xy, torch.where(hit[:, None, None], m, torch.zeros_like(m)),
                torch.where(hit, scale, torch.zeros_like(scale)))

    def payload(self, local_idx, feature_dist, full_xy_dists=None, query_xy=None):
        """``top_n.retrieve``'s output list [top_i, top_g_dists, top_f_dists, gt_i, gt_g_dist, ref_idx]
        (evaluation/top-n.py:110-119) from the hits of ``query_thinned`` for every query, in order, and
        either the queries' geographic distances to ALL references [Q, M] (``full_xy_dists``: the
        reference's table, read bit for bit) or the queries' positions [Q, 2] (``query_xy``: hit
        distances and ground truth from the index's own positions on the device, evaluation/geo.py —
        the direct form ``sqrt(dx*dx + dy*dy)``; a missing hit, row -1, is index -1 and distance inf)."""
        ref_idx = self.ref_idx
        if query_xy is not None:
            if full_xy_dists is not None:
                raise ValueError('payload takes full_xy_dists or query_xy, not both')
            if self._index is None:
                raise ValueError('query_xy needs the resident index: a Localizer made with query_fn has '
                                 'no device positions')
            from .top_n import device_ground_truth
            hits = torch.from_numpy(np.ascontiguousarray(local_idx, dtype=np.int64)).to(self.device)
            top_i, top_g_dists, gt_i, gt_g_dist = device_ground_truth(
                self._index.positions, query_xy, hits, ref_idx)
            return [top_i, top_g_dists, np.asarray(feature_dist, dtype=np.float64), gt_i, gt_g_dist, ref_idx]
        if full_xy_dists is None:
            raise ValueError('payload needs full_xy_dists or query_xy')
        xy_dists = np.asarray(full_xy_dists)[:, ref_idx]
        top_i = np.asarray(local_idx).astype(int)
        num_q = top_i.shape[0]
        top_g_dists = [[xy_dists[q, r] for r in top_i[q, :]] for q in range(num_q)]
        gt_i = np.argmin(xy_dists, axis=1)
        gt_g_dist = np.min(xy_dists, axis=1)
        top_i = [[ref_idx[r] for r in top_i[q, :]] for q in range(num_q)]
        gt_i = [ref_idx[r] for r in gt_i]
        return [top_i, top_g_dists, np.asarray(feature_dist, dtype=np.float64), gt_i, gt_g_dist, ref_idx]


def localize_set(loc, query_f, full_xy_dists=None, batch=1, prior_radius=0.0, stats=None, query_xy=None):
    """Feed the rows of query_f through ``loc`` in list order, ``batch`` at a time -> the payload
    (``Localizer.payload``: from the table ``full_xy_dists``, or from the positions ``query_xy``).

    ``prior_radius`` > 0: every call but the first searches within that many metres of the position
    estimate (first hit) of the last frame of the call before; a frame whose window holds fewer
    than n references is searched again without a window.  ``stats['researched']`` counts those."""
    batch = max(int(batch), 1)
    dists, idxs = [], []
    prior, again = None, 0
    for s in range(0, len(query_f), batch):
        rows = query_f[s:s + batch]
        if prior_radius > 0 and prior is not None:
            d, i = loc.query_thinned(rows, prior, prior_radius)
            short = np.nonzero(i[:, -1] < 0)[0]
            if len(short):
                d[short], i[short] = loc.query_thinned(rows[short])
                again += len(short)
        else:
            d, i = loc.query_thinned(rows)
        prior = loc.ref_xy[loc._orig[i[-1, 0]]]
        dists.append(d)
        idxs.append(i)
    if stats is not None:
        stats['researched'] = again
    return loc.payload(np.concatenate(idxs), np.concatenate(dists), full_xy_dists, query_xy)


class _SklearnRows:
    """scikit-learn's PCA behind the ``transform_rows`` interface (``--pca_backend sklearn``)."""

    def __init__(self, pca):
        self._pca = pca

    def transform_rows(self, x):
        x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        return self._pca.transform(x).astype(np.float32)


def main_parser():
    """The flags of ``main``."""
    import argparse
    from .top_n import GEO_ROUTES
    p = argparse.ArgumentParser()
    p.add_argument('--pca_lv_pickle', required=True)
    p.add_argument('--query_lv_pickle', required=True)
    p.add_argument('--ref_lv_pickle', required=True)
    p.add_argument('--query_csv', required=True)
    p.add_argument('--ref_csv', required=True)
    p.add_argument('--N', default=25, type=int)
    p.add_argument('--out_root', default='./scl_top_n')
    p.add_argument('--L', default=0.0, type=float, help='thinning distance in metres')
    p.add_argument('--D', default=256, type=int, help='PCA dimension (0: no whitening)')
    p.add_argument('--pca_backend', default='device', choices=['device', 'sklearn'])
    p.add_argument('--score', default='bf16x3', choices=['f32', 'bf16x3'],
                   help='nomination arithmetic of queries beyond the stream route (the lists are exact either way)')
    p.add_argument('--batch', default=1, type=int, help='frames per call')
    p.add_argument('--prior_radius', default=0.0, type=float,
                   help='metres around the previous call\'s last position estimate to search in (0: everywhere)')
    p.add_argument('--wide_index', default=0, type=int, choices=[0, 1],
                   help='1: descriptors wider than 256 columns get the resident wide index (needs --score f32); '
                        '0: every call on them is a one-shot top-n and --prior_radius is refused')
    p.add_argument('--geo', default='table', choices=list(GEO_ROUTES),
                   help='geographic distances: read out of the [Q, M] table of the reference, or computed from '
                        'the index\'s positions on the device (no table is built)')
    return p


def main(argv=None, query_fn=None):
    """The flags of ``top_n.main`` with a single --L and --D (0: no whitening), plus --batch: the
    query descriptors go through a ``Localizer`` in list order, --batch at a time; the payload of
    ``top_n.main`` goes to ``top_n.out_pickle_path``.  --prior_radius M (0: off) searches every call but
    the first within M metres of the call before's last position estimate (``localize_set``).
    --wide_index 1 keeps descriptors wider than 256 columns in the resident wide index
    (``RetrievalIndex(wide='resident')``; 0, the default: as before).
    --geo device takes the payload's geographic part from the index's positions (``Localizer.payload``
    with ``query_xy``) and builds no [Q, M] table; it needs the resident index, so together with
    ``query_fn`` it raises.  Prints queries per second, how many queries needed the exact fallback
    and, with a prior, how many frames were searched a second time.  Returns the path written (None:
    fewer than N references)."""
    import os
    import time
    from ..util import io
    from ..util.meta import get_xy
    from .pca import PCAWhitening
    flags = main_parser().parse_args(argv)
    if flags.geo == 'device' and query_fn is not None:
        raise ValueError('--geo device needs the resident index; query_fn (the CPU stand-in) has none')
    out = out_pickle_path(flags.out_root, flags.query_lv_pickle, flags.L, flags.D)
    if os.path.exists(out):
        print('{} already exists. Skipping.'.format(out))
        return out
    full_ref_xy = get_xy(io.load_csv(flags.ref_csv))
    full_query_xy = get_xy(io.load_csv(flags.query_csv))
    full_ref_f = np.array(io.load_pickle(flags.ref_lv_pickle), dtype=np.float32)
    full_query_f = np.array(io.load_pickle(flags.query_lv_pickle), dtype=np.float32)
    full_xy_dists = None
    if flags.geo == 'table':
        from sklearn.metrics import pairwise_distances
        full_xy_dists = pairwise_distances(full_query_xy, full_ref_xy, metric='euclidean')
    pca = None
    if flags.D > 0:
        pca_f = np.array(io.load_pickle(flags.pca_lv_pickle), dtype=np.float32)
        if flags.pca_backend == 'device':
            pca = PCAWhitening(flags.D, device='cuda').fit(pca_f)
        else:
            from sklearn.decomposition import PCA
            pca = _SklearnRows(PCA(whiten=True, n_components=flags.D).fit(pca_f))
    if len(thin_reference(full_ref_xy, flags.L)) < flags.N:       # (evaluation/top-n.py:96-97)
        return None
    loc = Localizer(full_ref_f, full_ref_xy, pca=pca, n=flags.N, l=flags.L, score=flags.score,
                    query_fn=query_fn, wide='resident' if flags.wide_index else 'delegate')
    if query_fn is None:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = {}
    payload = localize_set(loc, full_query_f, full_xy_dists, flags.batch, flags.prior_radius, stats,
                           full_query_xy if flags.geo == 'device' else None)
    dt = time.perf_counter() - t0
    os.makedirs(os.path.dirname(out), exist_ok=True)
    io.save_pickle(payload, out)
    print('{} queries, {} per call: {:.1f} queries/s, uncertified {}'.format(
        len(full_query_f), max(flags.batch, 1), len(full_query_f) / max(dt, 1e-9), loc.uncertified))
    if flags.prior_radius > 0:
        print('prior radius {:g} m: {} frames searched again without it'.format(
            flags.prior_radius, stats['researched']))
    return out


if __name__ == '__main__':
    main()

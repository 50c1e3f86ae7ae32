"""Shared by tests/test_geo_eval_host.py and tests/test_gpu_geo_eval.py: the golden run of the
reference's evaluation/top-n.py and the bound on what its expanded-form table may differ by."""
import base64
import json
import os

import numpy as np

from tests import util_data as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_ref_topn_v1.json')
U53 = 2.0 ** -53


def golden_run():
    """(case, data set, arrays) of tests/golden/golden_ref_topn_v1.json: the reference's own run of
    evaluation/top-n.py on tests/util_data.retrieval_dataset."""
    doc = json.load(open(GOLDEN))
    c = doc['cases'][0]
    ds = U.retrieval_dataset(seed=c['seed'], n_pca=c['n_pca'], n_ref=c['n_ref'], n_query=c['n_query'], e=c['e'])
    shp = c['top_i_shape']
    want = {'top_i': np.frombuffer(base64.b64decode(c['top_i_i32_b64']), '<i4').reshape(shp),
            'top_g': np.frombuffer(base64.b64decode(c['top_g_dists_f64_b64']), '<f8').reshape(shp),
            'gt_i': np.frombuffer(base64.b64decode(c['gt_i_i32_b64']), '<i4'),
            'gt_g': np.frombuffer(base64.b64decode(c['gt_g_dist_f64_b64']), '<f8')}
    return c, ds, want


def expanded_form_bound(query_xy, ref_xy_of_pairs, dist):
    """Bound on |dist_table^2 - dist_direct^2| for pairs (query row, its reference), see
    tests/test_geo_eval_host.py::test_golden_ground_truth_within_the_expanded_forms_own_error
    for the count: 8 u (|q|^2 + |r|^2) for the table's expanded form, 8 u d2 for the direct form and for
    comparing stored distances through their squares."""
    q2 = (np.asarray(query_xy) ** 2).sum(-1)
    r2 = (np.asarray(ref_xy_of_pairs) ** 2).sum(-1)
    return 8.0 * U53 * (q2 + r2) + 8.0 * U53 * np.asarray(dist) ** 2

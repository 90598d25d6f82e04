"""GPU tests (-m gpu) of the own-means lane of the Gram pass (stats_gram_own_kernel, csrc/stats_gram.hip) on data where
every result is exact, so that the comparison needs no tolerance and does not depend on the order of any sum.

X holds integers in [-8, 8] and m is 128 or 256, a power of two.  Then, in float64,
  * a row sum is an integer of magnitude <= 8 m and the row mean, rowsum / m, is exact;
  * a centred value x - mean = (m x - rowsum) / m is a multiple of 1/m of magnitude <= 16: exact;
  * a product of two of them is a multiple of 1/m^2 below 2^8, i.e. an integer below 2^24 over m^2 = 2^16: exact;
  * a sum of at most 2^14 such products stays below 2^38 over 2^16: every partial sum is exact, in any order.
So G m^2 must EQUAL D^T D with the integer matrix D = m x - rowsum, and the means must equal rowsum / m.

The reference is formed in int64.  D^T D itself goes through a float64 matrix product, which is exact for the same reason
(|D| <= 2^12, partial sums < 2^38 < 2^53), and is converted back; the first columns are checked against a pure int64
product as well (a full int64 product of this size takes NumPy several seconds).

Row counts per feature: 1, 31, 33, 8192 + 5 and 3 x 3000.  A panel has 32 rows at both widths, and a feature with fewer
panels than workgroups gets one workgroup per panel: 1 and 31 rows are a single partial panel, 33 rows a full and a
partial one in two workgroups.  8197 rows are 257 panels, the last one partial: with one workgroup per CU (m = 256) some
workgroup takes a second panel through the pipeline, with two per CU (m = 128) every panel has its own.  3 x 3000 rows
are 94 panels per feature (the last partial) over fewer workgroups at m = 256: one and two panels side by side, in
three features."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (31, 1), (33, 1), (8192 + 5, 1), (3000, 3)]


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine()


def _reference(Xi, n_points, F, m):
    """-> (row sums, per-feature D^T D) as int64"""
    rowsum = Xi.sum(axis=1)
    D = m * Xi - rowsum[:, None]
    assert np.abs(D).max() <= 16 * m
    G = np.empty((F, m, m), dtype=np.int64)
    for f in range(F):
        Df = D[f * n_points:(f + 1) * n_points]
        Dd = Df.astype(np.float64)
        Gd = Dd.T @ Dd
        G[f] = Gd.astype(np.int64)
        assert np.array_equal(G[f].astype(np.float64), Gd)
        assert np.array_equal(G[f][:4], Df[:, :4].T @ Df)              # pure int64 on the first rows
    return rowsum, G


@pytest.mark.parametrize('m', [128, 256])
@pytest.mark.parametrize('n_points,F', CASES)
def test_gram_and_means_are_exact(eng, n_points, F, m):
    rng = np.random.default_rng(1000 * m + n_points)
    n = n_points * F
    Xi = rng.integers(-8, 9, size=(n, m)).astype(np.int64)
    rowsum, G_ref = _reference(Xi, n_points, F, m)
    X = eng.to_device(Xi.astype(np.float64))
    assert X.data_ptr() % 16 == 0 and X.stride(0) == m              # the layout the own-means lane takes
    rowmean, fstats, gram = eng.stats_gram(X, 0, n_points, F, center=True)
    mean_h, gram_h, fstats_h = eng.to_host(rowmean), eng.to_host(gram), eng.to_host(fstats)
    assert np.array_equal(mean_h * m, rowsum.astype(np.float64))
    got = gram_h * float(m * m)
    assert np.array_equal(got, np.rint(got))                           # integers: the scaling by m^2 is exact
    assert np.array_equal(got.astype(np.int64), G_ref)
    assert np.array_equal(fstats_h[:, 0], np.full(F, float(n_points)))

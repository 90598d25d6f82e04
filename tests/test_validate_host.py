"""ROM.transform / ROM.reconstruction_error on the CPU: the public methods over a NumPy double of the two engine calls
(HipEngine.encode / field_error, csrc/validate.hip, held to NumPy in tests/test_validate_gpu.py), against plain NumPy on the
object's own host arrays.

Bars.  Everything here is f64 NumPy against f64 NumPy in another summation order, so the worst-case bound of a sum of n
products in ANY order applies (Higham, Accuracy and Stability, (3.5)):  |fl(sum) - sum| <= gamma_n sum |terms|,
gamma_n ~ n eps.
 * transform: an entry lies within  gamma sum_i |Ur[i, c] x0[i, j]|,  gamma = (n + r + 4) eps  (n products, the rounding of
   x0 itself: one subtraction and one division, and slack for the last additions).
 * reconstruction_error: per row  |delta_i| <= (r + 6) eps (|X_cnt_i| + |X_true_ij| + X_scl sum_c |Ur[i, c] a_c|)  for the
   field value and the difference; then  sse  within  2 sqrt(sse) |delta|_2 + |delta|_2^2 + gamma sse,  ss_true  within
   gamma ss_true,  max_abs  within  max delta.  (error_bars below; the GPU test uses the same function.)
"""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from openmeasure_amd.sparse_sensing import ROM
from tests.numpy_engine import NumpyEngine
from tests.test_cols_host import _free_port, make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53                                              # unit roundoff of f64


def numpy_encode(U, row0, n_points, F, mu, scale, X, dtype=np.float64):
    """-> (A (k, r), S (k, r) = sum_i |Ur[i, c] x0[i, j]|): the host formula  Ur.T @ ((x - cnt) / scl), transposed"""
    feat = np.minimum((row0 + np.arange(U.shape[0])) // n_points, F - 1)
    x0 = (X.astype(np.float64) - mu[:, None]) / scale[feat][:, None]
    U = U.astype(dtype)
    return (x0.astype(dtype).T @ U), (np.abs(x0).astype(dtype).T @ np.abs(U))


def numpy_field_error(U, row0, n_points, F, mu, scale, A, Xt, dtype=np.float64):
    """-> dict: rec (k, F, 4) as HipEngine.field_error returns it, delta (n, k) the per-row rounding bound of d,
    d (n, k), feat (n,)"""
    n = U.shape[0]
    feat = np.minimum((row0 + np.arange(n)) // n_points, F - 1)
    U, Xt, A = U.astype(dtype), Xt.astype(dtype), A.astype(dtype)
    sc, mu = scale.astype(dtype)[feat][:, None], mu.astype(dtype)[:, None]
    d = (U @ A.T) * sc + mu - Xt
    delta = (U.shape[1] + 6) * EPS * (np.abs(mu) + np.abs(Xt) + sc * (np.abs(U) @ np.abs(A).T))
    rec = np.zeros((A.shape[0], F, 4), dtype=dtype)
    rec[:, :, 3] = -1
    for f in range(F):
        sel = np.flatnonzero(feat == f)
        if len(sel):
            ad = np.abs(d[sel])
            rec[:, f, 0] = (d[sel] ** 2).sum(axis=0)
            rec[:, f, 1] = (Xt[sel] ** 2).sum(axis=0)
            rec[:, f, 2] = ad.max(axis=0)
            rec[:, f, 3] = row0 + sel[ad.argmax(axis=0)]       # argmax: the first = lowest row
    return dict(rec=rec, delta=delta, d=d, feat=feat)


def error_bars(ref, n, r):
    """(sse, ss_true, max_abs) bars of the module docstring from numpy_field_error's output, each (k, F)"""
    gamma = (n + r + 4) * EPS
    rec, delta, feat = ref['rec'].astype(np.float64), ref['delta'].astype(np.float64), ref['feat']
    k, F = rec.shape[:2]
    b_sse, b_max = np.zeros((k, F)), np.zeros((k, F))
    for f in range(F):
        sel = feat == f
        if sel.any():
            dn = np.sqrt((delta[sel] ** 2).sum(axis=0))
            b_sse[:, f] = 2 * np.sqrt(rec[:, f, 0]) * dn + dn * dn + gamma * rec[:, f, 0]
            b_max[:, f] = delta[sel].max(axis=0)
    return b_sse, gamma * rec[:, :, 1], b_max


class ValidateNumpyEngine(NumpyEngine):
    """NumpyEngine + NumPy encode / field_error with the contracts of HipEngine's"""

    def encode(self, Ur, row0, n_points, n_features, rowmean, scale, X_new):
        assert X_new.dim() == 2 and X_new.shape[0] == Ur.shape[0]
        A, _ = numpy_encode(self._w(Ur), row0, n_points, n_features, rowmean.numpy(), scale.numpy(), self._w(X_new))
        return torch.from_numpy(np.ascontiguousarray(A))

    def field_error(self, Ur, row0, n_points, n_features, rowmean, scale, A, X_true):
        assert X_true.dim() == 2 and tuple(A.shape) == (X_true.shape[1], Ur.shape[1])
        ref = numpy_field_error(self._w(Ur), row0, n_points, n_features, rowmean.numpy(), scale.numpy(), A.numpy(),
                                self._w(X_true))
        return torch.from_numpy(np.ascontiguousarray(ref['rec']))


def fitted(case, engine=None, **kw):
    rom = ROM(case['X'], case['F'], None, engine=engine or ValidateNumpyEngine())
    rom.fit(select_modes='number', n_modes=case['r'], **kw)
    return rom


def held_out(case):
    return np.stack(case['truth'], axis=1)                    # (n, 3) fields that are not columns of X


def host_transform(rom, Xn):
    """plain NumPy on the object's host arrays -> (A, S)"""
    x0 = (np.asarray(Xn, dtype=np.float64) - rom.X_cnt) / rom.X_scl
    U = np.asarray(rom.Ur, dtype=np.float64)
    return x0.T @ U, np.abs(x0).T @ np.abs(U)


def check_transform(rom, Xn, A):
    ref, S = host_transform(rom, Xn)
    n, r = np.asarray(rom.Ur).shape
    assert A.shape == ref.shape and A.dtype == np.float64 and isinstance(A, np.ndarray)
    excess = np.abs(A - ref) / ((n + r + 4) * EPS * S)
    print('transform: worst error / bar', excess.max())
    assert excess.max() <= 1.0


def check_errors(rom, Xt, A, err):
    """reconstruction_error's dict against NumPy on the object's reconstruct(A) field"""
    Xt = np.asarray(Xt, dtype=np.float64)
    field = rom.reconstruct(A)
    F, n_pt = rom.n_features, rom.n_points
    U = np.asarray(rom.Ur, dtype=np.float64)
    ref = numpy_field_error(U, 0, n_pt, F, rom.X_cnt[:, 0], rom._scl_f, np.atleast_2d(A), Xt)
    b_sse, b_sst, b_max = error_bars(ref, *U.shape)
    d = field - Xt
    for f in range(F):
        blk = slice(f * n_pt, (f + 1) * n_pt)
        assert np.all(np.abs((d[blk] ** 2).sum(axis=0) - err['sse'][:, f]) <= 2 * b_sse[:, f])   # two computed values: 2 x
        assert np.all(np.abs((Xt[blk] ** 2).sum(axis=0) - err['ss_true'][:, f]) <= 2 * b_sst[:, f])
        assert np.all(np.abs(np.abs(d[blk]).max(axis=0) - err['max_abs'][:, f]) <= 2 * b_max[:, f])
        rows = err['max_row'][:, f]
        assert np.all((rows >= f * n_pt) & (rows < (f + 1) * n_pt))
        for j, row in enumerate(rows):                         # the row it names attains the maximum (to rounding)
            assert abs(d[row, j]) >= np.abs(d[blk, j]).max() - 2 * b_max[j, f]
    assert err['max_row'].dtype == np.int64
    np.testing.assert_array_equal(err['rel_l2'], np.sqrt(err['sse'] / err['ss_true']))
    np.testing.assert_array_equal(err['rmse'], np.sqrt(err['sse'] / n_pt))
    np.testing.assert_array_equal(err['rel_l2_total'], np.sqrt(err['sse'].sum(axis=1) / err['ss_true'].sum(axis=1)))
    assert set(err) == {'sse', 'ss_true', 'max_abs', 'max_row', 'rel_l2', 'rmse', 'rel_l2_total'}
    k = Xt.shape[1]
    assert all(err[key].shape == (k, F) for key in ('sse', 'ss_true', 'max_abs', 'max_row', 'rel_l2', 'rmse'))
    assert err['rel_l2_total'].shape == (k,)


@pytest.mark.parametrize('axis_cnt', [1, None])
def test_transform_and_error_against_numpy(axis_cnt):
    case = make_case(seed=4, n_points=350, F=3, m=20, r=7, offset=0.5)
    rom = fitted(case, axis_cnt=axis_cnt)
    Xn = held_out(case)
    A = rom.transform(Xn)
    check_transform(rom, Xn, A)
    # 1-D input: one snapshot -> (1, r)
    a1 = rom.transform(Xn[:, 1])
    assert a1.shape == (1, case['r'])
    check_transform(rom, Xn[:, 1:2], a1)
    # the snapshots of the fit come back as Ar (orthonormal basis): a looser, conditioning-dependent statement, so only
    # to the accuracy of the Gram route
    np.testing.assert_allclose(rom.transform(case['X']), rom.Ar, rtol=0, atol=1e-9 * np.abs(rom.Ar).max())
    rng = np.random.default_rng(0)
    Ap = A + 0.01 * rng.standard_normal(A.shape)
    check_errors(rom, Xn, Ap, rom.reconstruction_error(Xn, Ap))
    e1 = rom.reconstruction_error(Xn[:, 2], Ap[2])            # (n,) and (r,)
    check_errors(rom, Xn[:, 2:3], Ap[2:3], e1)
    # Ar=None: the truncation error of the basis = the error at transform's coefficients
    e0 = rom.reconstruction_error(Xn)
    check_errors(rom, Xn, A, e0)


def test_float32_input_and_device_tensors():
    case = make_case(seed=5, n_points=300, F=2, m=16, r=5)
    rom = fitted(case)
    Xn = held_out(case)
    X32 = Xn.astype(np.float32)
    seen = []
    enc = rom._eng.encode
    rom._eng.encode = lambda *a: (seen.append(a[-1].dtype), enc(*a))[1]
    A32 = rom.transform(X32)
    assert seen == [torch.float32]                            # uploaded as stored, widened by the engine
    check_transform(rom, X32.astype(np.float64), A32)
    check_errors(rom, X32.astype(np.float64), A32, rom.reconstruction_error(X32, A32))
    # a "device" tensor and a DeviceMatrix are used in place
    from openmeasure_amd.rom import DeviceMatrix
    t = torch.from_numpy(Xn.copy())
    np.testing.assert_array_equal(rom.transform(t), rom.transform(Xn))
    np.testing.assert_array_equal(rom.transform(DeviceMatrix(t)), rom.transform(Xn))
    np.testing.assert_array_equal(rom.transform(t[:, 0]), rom.transform(Xn[:, 0].copy()))
    e_t, e_h = rom.reconstruction_error(DeviceMatrix(t), A32), rom.reconstruction_error(Xn, A32)
    for key in e_h:
        np.testing.assert_array_equal(e_t[key], e_h[key])


def test_foreign_basis():
    """fit(basis=...) and an assigned Ur: transform is Ur^T x0 for whatever basis the object holds"""
    case = make_case(seed=6, n_points=250, F=2, m=18, r=6)
    other = fitted(case)
    rng = np.random.default_rng(1)
    B = np.asarray(other.Ur) @ (np.eye(case['r']) + 0.3 * rng.standard_normal((case['r'], case['r'])))   # not orthonormal
    rom = ROM(case['X'], case['F'], None, engine=ValidateNumpyEngine())
    rom.fit(basis=(B, np.asarray(other.Ar)))
    Xn = held_out(case)
    A = rom.transform(Xn)
    check_transform(rom, Xn, A)
    check_errors(rom, Xn, A, rom.reconstruction_error(Xn, A))
    other.Ur = B
    check_transform(other, Xn, other.transform(Xn))


def test_full_rank_reconstruction_is_exact_to_rounding():
    """r = m - 1 keeps every direction of the row-centred X0 (rank m - 1): reconstruct(Ar) is X.  The Gram route leaves the
    basis with a relative error of eps kappa^2 (rom.py, _GRAM_KAPPA_REFINE), a field value is a sum of r products and the
    error norms are relative to |X|: bar = 64 m eps kappa^2, the 64 for the constants of the eigen-solve and the three
    passes (Gram, projection, reconstruction) the values went through.  kappa = 1.3 for this Gaussian matrix."""
    rng = np.random.default_rng(11)
    n_pt, F, m = 300, 2, 8
    X = rng.standard_normal((n_pt * F, m)) + 3.0
    rom = ROM(X, F, None, engine=ValidateNumpyEngine())
    rom.fit(select_modes='number', n_modes=m - 1)
    kappa = rom.Sigma_r.max() / rom.Sigma_r.min()
    assert kappa < 2.0                                        # well conditioned
    err = rom.reconstruction_error(X, rom.Ar)
    bar = 64 * m * 2 * EPS * kappa ** 2
    print('full rank: rel_l2', err['rel_l2'].max(), 'total', err['rel_l2_total'].max(), 'bar', bar)
    assert err['rel_l2'].max() <= bar and err['rel_l2_total'].max() <= bar
    assert err['max_abs'].max() <= bar * np.abs(X).max() * np.sqrt(n_pt)


def test_refusals():
    case = make_case(seed=7, n_points=200, F=2, m=12, r=4)
    rom = fitted(case)
    Xn = held_out(case)
    n = Xn.shape[0]
    for bad in (Xn[:-1], Xn[:-1, 0], np.zeros((n + 1, 2), dtype=np.float32)):
        with pytest.raises(ValueError, match='rows'):
            rom.transform(bad)
        with pytest.raises(ValueError, match='rows'):
            rom.reconstruction_error(bad)
    with pytest.raises(ValueError):
        rom.transform(np.zeros((n, 2, 2)))
    A = rom.transform(Xn)
    with pytest.raises(ValueError, match='Ar has shape'):
        rom.reconstruction_error(Xn, A[:2])
    with pytest.raises(ValueError, match='Ar has shape'):
        rom.reconstruction_error(Xn, A[:, :-1])
    unfit = ROM(case['X'], case['F'], None, engine=ValidateNumpyEngine())
    with pytest.raises(AttributeError, match="no attribute 'Ur'"):
        unfit.transform(Xn)
    with pytest.raises(AttributeError, match="no attribute 'Ur'"):
        unfit.reconstruction_error(Xn)
    plain = fitted(case, engine=NumpyEngine())                # no encode / field_error: no CPU fallback
    with pytest.raises(NotImplementedError, match='encode'):
        plain.transform(Xn)
    with pytest.raises(NotImplementedError, match='field_error'):
        plain.reconstruction_error(Xn, A)
    with pytest.raises(NotImplementedError):
        plain.reconstruction_error(Xn)


def test_transform_flushes_a_deferred_reconstruct():
    case = make_case(seed=7, n_points=200, F=2, m=12, r=4)
    rom = fitted(case)
    pf = rom.reconstruct(rom.Ar[:1], to_host=False, wait=False)
    assert not pf.launched
    rom.transform(held_out(case))
    assert pf.launched


# ------------------------------------------------------------------------------------------------------ sharded, over gloo
SHARD_CASE = dict(seed=2, n_points=300, F=3, m=32, r=10)      # 900 rows, features of 300


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from openmeasure_amd.sparse_sensing import ROM, RowShard
        from tests.test_cols_host import make_case
        from tests.test_validate_host import SHARD_CASE, ValidateNumpyEngine, held_out
        case = make_case(**SHARD_CASE)
        n = case['X'].shape[0]
        cuts = [0, 400, n]                                     # cut INSIDE feature 1
        row0, n_loc = cuts[rank], cuts[rank + 1] - cuts[rank]
        rom = ROM(np.ascontiguousarray(case['X'][row0:row0 + n_loc]), case['F'], None, shard=RowShard(row0, n),
                  engine=ValidateNumpyEngine())
        rom.fit(select_modes='number', n_modes=case['r'])
        Xn = np.ascontiguousarray(held_out(case)[row0:row0 + n_loc])
        calls = []
        ar, ag = rom._all_reduce, rom._all_gather
        rom._all_reduce = lambda t: (calls.append('reduce'), ar(t))[1]
        rom._all_gather = lambda t: (calls.append('gather'), ag(t))[1]
        A = rom.transform(Xn)
        Ap = A + 0.01 * np.random.default_rng(0).standard_normal(A.shape)
        e_p, e_0 = rom.reconstruction_error(Xn, Ap), rom.reconstruction_error(Xn)
        with open(os.path.join(out_dir, f'rank{rank}.pkl'), 'wb') as fh:
            pickle.dump(dict(A=A, e_p=e_p, e_0=e_0, calls=calls, Ur=np.asarray(rom.Ur, dtype=np.float64),
                             cnt=np.asarray(rom.X_cnt)[:, 0], scl=np.asarray(rom._scl_f)), fh)
    finally:
        dist.destroy_process_group()


def test_sharded_over_gloo(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = []
    for q in range(2):
        with open(tmp_path / f'rank{q}.pkl', 'rb') as fh:
            got.append(pickle.load(fh))
    case = make_case(**SHARD_CASE)
    Xn = held_out(case)
    n, F, n_pt, r = Xn.shape[0], case['F'], case['n_points'], case['r']
    # every rank holds the same answers
    np.testing.assert_array_equal(got[0]['A'], got[1]['A'])
    for name in ('e_p', 'e_0'):
        for key in got[0][name]:
            np.testing.assert_array_equal(got[0][name][key], got[1][name][key])
    assert got[0]['calls'] == ['reduce', 'gather', 'reduce', 'gather']     # transform | error | error with Ar=None
    # ... the single-process values for the ranks' own basis, centre and scale, at the bars of the module docstring
    U, cnt, scl = np.vstack([g['Ur'] for g in got]), np.concatenate([g['cnt'] for g in got]), got[0]['scl']
    ref, S = numpy_encode(U, 0, n_pt, F, cnt, scl, Xn)
    assert np.all(np.abs(got[0]['A'] - ref) <= (n + r + 4) * EPS * S)
    Ap = got[0]['A'] + 0.01 * np.random.default_rng(0).standard_normal(got[0]['A'].shape)
    for A, e in ((Ap, got[0]['e_p']), (got[0]['A'], got[0]['e_0'])):
        rf = numpy_field_error(U, 0, n_pt, F, cnt, scl, A, Xn)
        b_sse, b_sst, b_max = error_bars(rf, n, r)
        assert np.all(np.abs(e['sse'] - rf['rec'][:, :, 0]) <= 2 * b_sse)
        assert np.all(np.abs(e['ss_true'] - rf['rec'][:, :, 1]) <= 2 * b_sst)
        assert np.all(np.abs(e['max_abs'] - rf['rec'][:, :, 2]) <= 2 * b_max)
        np.testing.assert_array_equal(e['max_row'], rf['rec'][:, :, 3].astype(np.int64))   # global rows, feature 1 is cut
        np.testing.assert_array_equal(e['rmse'], np.sqrt(e['sse'] / n_pt))                  # the GLOBAL n_points
    # ... and the single-process object: the truncation error depends on the subspace alone, which the two fits (Gram sums in
    # another order) give to eps kappa^2 -- 1e-9 is far above that and far below any mistake in the merge
    rom = fitted(case)
    e_s = rom.reconstruction_error(Xn)
    for key in ('sse', 'ss_true', 'max_abs', 'rel_l2', 'rmse', 'rel_l2_total'):
        np.testing.assert_allclose(got[0]['e_0'][key], e_s[key], rtol=1e-9)
    np.testing.assert_array_equal(got[0]['e_0']['max_row'], e_s['max_row'])

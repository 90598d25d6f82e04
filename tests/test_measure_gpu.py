"""csrc/measure.hip and the sampled consumers of its results on the device, held to the longdouble references and the bars of
tests/test_measure_host.py (derived there, before any run on a GPU).  Every kernel call runs twice and the two results are
compared bit for bit.

  * measure_csr: every width at which the kernel takes another path (second accumulator from 65 columns, column groups of 128),
    both storage types of the basis, a contiguous basis and a column view, with and without scl, three row shards whose cuts lie
    inside features; |got - ref| <= (ceil(L / 4) + 4) 2^-53 T entrywise, exact zeros where T == 0, exact gathers for one-hot rows.
  * properties with no tolerance: the first column group of a wide basis equals the call on those columns alone; cnt and scl do
    not depend on the width; an f32 basis gives the bits of the same basis widened; permuting the rows of C permutes the
    results; a row inside a shard gives the bits of the whole matrix; a C without stored entries gives zeros.
  * eng.reconstruct(rowscale=) as reconstruct(sampling=) calls it, on Theta-shaped matrices that fill 16-row MFMA blocks and 64-row
    panels and do not: |got - ref| <= (r + 4) 2^-53 (|rs_i| sum_k |a_pk u_ik| + |mu_i|); the columns of out= beyond s keep
    their bytes.
  * the public surface -- train, unscale_data(sampling=), reconstruct(sampling=), DeviceCSR.dot -- with C as an ndarray, a
    scipy.sparse matrix with unsorted indices and a DeviceCSR: the same bits, within the propagated bars.
The worst error / bar ratio of every test is printed (pytest -s shows it)."""
import numpy as np
import pytest

from openmeasure_amd.sparse_sensing import SPR, DeviceCSR
from tests.test_measure_host import (CASES, LD, N, N_FEATURES, N_POINTS, ROWMEAN, ROWS, SCALE, SHARDS, U53, WHOLE, WIDTHS_F32,
                                     basis, check_measure, check_reconstruct, host, measure, measure_bar, public_rows,
                                     reconstruct_bar, reconstruct_inputs, ref_measure, ref_reconstruct, reference, row_kinds,
                                     run_case, take_rows, upload_csr)

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def same_bits(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())
               for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_measure(eng, case):
    _, worst = run_case(eng, case, twice=True)
    print(f'measure {case.name}: worst error / bar = {worst:.3f}')
    WORST[f'measure {case.name}'] = worst


def test_column_groups(eng):
    """128 columns per launch: what the first launch writes does not depend on the launches after it, and cnt / scl, which every
    launch writes again, come out the same whatever the width"""
    wide = measure(eng, ROWS, basis(257), twice=True)
    first = measure(eng, ROWS, basis(128), pad=257 - 128, twice=True)          # the view Ur[:, :128] of a 257-column matrix
    assert wide[0][:, :128].tobytes() == first[0].tobytes()
    none = measure(eng, ROWS, None, twice=True)
    for r in (1, 64, 65, 128, 129, 256, 257):
        got = wide if r == 257 else measure(eng, ROWS, basis(r))
        assert same_bits(got[1:], none[1:]), r
        assert np.ascontiguousarray(wide[0][:, :r]).tobytes() == got[0].tobytes(), r     # columns do not interact either


@pytest.mark.parametrize('r', WIDTHS_F32)
def test_f32_basis_is_the_widened_basis(eng, r):
    """the conversion on load is exact and the arithmetic behind it is the same"""
    U32 = basis(r, f32=True)
    assert same_bits(measure(eng, ROWS, U32, twice=True), measure(eng, ROWS, U32.astype(np.float64), twice=True))


def test_rows_do_not_interact(eng):
    order = np.random.default_rng(3).permutation(len(ROWS.names))
    assert not np.array_equal(order, np.arange(len(order)))
    for U in (basis(129), None):
        a, b = measure(eng, ROWS, U, twice=True), measure(eng, take_rows(ROWS, order), U, twice=True)
        assert same_bits([None if x is None else x[order] for x in a], b)


@pytest.mark.parametrize('r', [0, 129])
def test_shards(eng, r):
    U = basis(r)
    whole, ref_whole = measure(eng, ROWS, U, twice=True), reference(ROWS, U)
    total = [None if x is None else np.zeros(x.shape, dtype=LD) for x in whole]
    worst = 0.0
    for shard in SHARDS:
        row0, n_rows = shard
        got = measure(eng, ROWS, U, shard=shard, twice=True)
        worst = max(worst, check_measure(got, reference(ROWS, U, shard), f'shard {shard}'))
        kinds = np.array(row_kinds(ROWS, row0, n_rows))
        for g, w, tot in zip(got, whole, total):
            if g is None:
                continue
            tot += g
            assert g[kinds == 'inside'].tobytes() == w[kinds == 'inside'].tobytes(), shard      # every entry keeps its wave slot
            assert not g[(kinds == 'outside') | (kinds == 'empty')].any(), shard
        for name, i in zip(ROWS.names, range(len(kinds))):                        # the one-hot rows at the edges of this shard
            if name.startswith('one-hot'):
                col = int(ROWS.indices[ROWS.indptr[i]])
                if row0 <= col < row0 + n_rows:
                    assert got[1][i] == ROWMEAN[col] and got[2][i] == SCALE[col // N_POINTS], (shard, name)
                    assert r == 0 or np.array_equal(got[0][i], U[col]), (shard, name)
                else:
                    assert got[1][i] == 0 and got[2][i] == 0 and (r == 0 or not got[0][i].any()), (shard, name)
        assert {c for c in (row0 - 1, row0, row0 + n_rows - 1, row0 + n_rows) if 0 <= c < N} <= {
            int(ROWS.indices[ROWS.indptr[i]]) for i, name in enumerate(ROWS.names) if name.startswith('one-hot')}
    # each shard is within its bar of its share of the sum, the shares' T add up to the whole T, the whole is within its bar
    for key, w, tot in zip(('Theta', 'cnt', 'scl'), whole, total):
        if w is None:
            continue
        bar = 3 * measure_bar(ref_whole['L'], ref_whole['T_' + key])
        err = np.abs(tot - w.astype(LD))
        assert np.all(err[bar == 0] == 0) and np.all(err <= bar), key
        worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max(initial=0)))
    print(f'measure shards r = {r}: worst error / bar = {worst:.3f}')
    WORST[f'shards r={r}'] = worst


@pytest.mark.parametrize('r,f32', [(0, False), (3, False), (129, False), (65, True)])
def test_no_stored_entries(eng, r, f32):
    """indptr all zero, indices and vals empty: what scipy's C.dot gives -- zeros"""
    s = 5
    empty = take_rows(ROWS, [0] * s)
    assert empty.indptr.tolist() == [0] * (s + 1) and empty.indices.shape == (0,) and empty.vals.shape == (0,)
    for scl in (True, False):
        Th, cnt, sc = measure(eng, empty, basis(r, f32), scl=scl, twice=True)
        assert (Th is None) == (r == 0) and (r == 0 or (Th.shape == (s, r) and Th.dtype == np.float64 and not Th.any()))
        assert cnt.shape == (s,) and cnt.dtype == np.float64 and not cnt.any()
        assert (sc is None) == (not scl) and (sc is None or (sc.shape == (s,) and not sc.any()))


# ------------------------------------------------------------------------------------------------ sampled reconstruct
S_LIST = [1, 15, 16, 17, 63, 64, 65, 130]
R_F64 = [1, 13, 96, 97, 112, 128, 129]          # LDS panels; register-direct at 112 and 128; 129: a second column group accumulates
R_F32 = [16, 48, 128]                           # register-direct
NP_LIST = [1, 16, 17]                           # one pass of 16 vectors, not full, full, and a second pass
SENTINEL = -777.0


def device_basis(eng, U, even):
    """contiguous, or -- for an odd width -- padded to an even leading dimension the way ROM.reconstruct(sampling=) pads Theta"""
    t = eng.torch
    Ud = eng.to_device(U, dtype=t.float32 if U.dtype == np.float32 else t.float64)
    if even:
        Ud = t.nn.functional.pad(Ud, (0, 1))[:, :U.shape[1]]
        assert Ud.stride(0) == U.shape[1] + 1 and Ud.stride(0) % 2 == 0
    return Ud


def reconstruct_twice(eng, Ud, n_points, n_features, mu, scale, A, rowscale, pad=5):
    """-> (n_p, s) on the host, written through an out= view of a wider buffer whose other columns must keep their bytes"""
    t = eng.torch
    s, n_p = Ud.shape[0], A.shape[0]
    runs = []
    for _ in range(2):
        buf = t.full((n_p, s + pad), SENTINEL, dtype=t.float64, device=eng.device)
        out = eng.reconstruct(Ud, 0, n_points, n_features, mu, scale, A, out=buf[:, :s], rowscale=rowscale)
        assert out.data_ptr() == buf.data_ptr()
        runs.append(host(eng, buf))
    assert runs[0].tobytes() == runs[1].tobytes()
    assert np.all(runs[0][:, s:] == SENTINEL)
    return np.ascontiguousarray(runs[0][:, :s])


@pytest.mark.parametrize('s', S_LIST)
def test_reconstruct_with_rowscale(eng, s):
    """as ROM.reconstruct(sampling=) calls it: row0 = 0, n_points = s, one feature of scale 1, the rows' own scale in rowscale"""
    ones = eng.to_device(np.ones(1))
    worst, calls = 0.0, 0
    for f32, widths in ((False, R_F64), (True, R_F32)):
        for r in widths:
            for n_p in NP_LIST:
                U, A, rs, mu = reconstruct_inputs(s, r, n_p, f32)
                want, T = ref_reconstruct(U, A, rs, mu)
                A_d, rs_d, mu_d = eng.to_device(A), eng.to_device(rs), eng.to_device(mu)
                for even in (False, True) if r % 2 else (False,):
                    got = reconstruct_twice(eng, device_basis(eng, U, even), s, 1, mu_d, ones, A_d, rs_d)
                    worst = max(worst, check_reconstruct(got, want, T, r, (s, r, n_p, f32, even)))
                    calls += 1
    print(f'sampled reconstruct s = {s}: {calls} shapes, worst error / bar = {worst:.3f}')
    WORST[f'reconstruct s={s}'] = worst


@pytest.mark.parametrize('r,f32', [(13, False), (96, False), (112, False), (129, False), (48, True)])
def test_rowscale_spelt_out_is_the_feature_scale(eng, r, f32):
    """rowscale = scale[feature of the row] gives the bits of rowscale=None: the two differ only in where the factor is read"""
    s, n_points, n_p = 130, 65, 3
    U, A, _, mu = reconstruct_inputs(s, r, n_p, f32, seed=1)
    scale = np.array([0.5, -20.0])
    Ud = device_basis(eng, U, bool(r % 2))
    args = (eng.to_device(mu), eng.to_device(scale), eng.to_device(A))
    plain = reconstruct_twice(eng, Ud, n_points, 2, *args, None)
    spelt = reconstruct_twice(eng, Ud, n_points, 2, *args, eng.to_device(np.repeat(scale, n_points)))
    assert plain.tobytes() == spelt.tobytes()
    want, T = ref_reconstruct(U, A, np.repeat(scale, n_points), mu)
    WORST[f'feature scale r={r}'] = check_reconstruct(plain, want, T, r)


# ------------------------------------------------------------------------------------------------ the public surface
@pytest.fixture(scope='module')
def fitted(eng):
    """an SPR on a 600 x 12 matrix with three features of different size and offset, five modes, and the public rows of C in
    the three forms a caller may hand over"""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 6)) @ ((0.6 ** np.arange(6))[:, None] * rng.standard_normal((6, 12)))
    X += 1e-3 * rng.standard_normal(X.shape)
    for f, (size, offset) in enumerate(((1.0, 0.0), (40.0, -300.0), (5e-3, 2.0))):
        X[f * N_POINTS:(f + 1) * N_POINTS] = size * X[f * N_POINTS:(f + 1) * N_POINTS] + offset
    spr = SPR(X, N_FEATURES, None, engine=eng)
    spr.fit(select_modes='number', n_modes=5)
    pub = public_rows()
    s = len(pub.names)
    shuffled_ix, shuffled_v = pub.indices.copy(), pub.vals.copy()
    for i in range(s):
        lo, hi = pub.indptr[i], pub.indptr[i + 1]
        p = rng.permutation(hi - lo)
        shuffled_ix[lo:hi], shuffled_v[lo:hi] = pub.indices[lo:hi][p], pub.vals[lo:hi][p]
    dense = sp.csr_matrix((pub.vals, pub.indices, pub.indptr), shape=(s, N)).toarray()
    device = DeviceCSR(*upload_csr(eng, pub), (s, N), engine=eng)

    def forms():                                              # a fresh unsorted matrix every time: the library may sort what it is given
        unsorted = sp.csr_matrix((shuffled_v.copy(), shuffled_ix.copy(), pub.indptr.copy()), shape=(s, N))
        assert not np.array_equal(unsorted.indices, pub.indices) and not unsorted.has_sorted_indices
        return {'ndarray': dense, 'scipy unsorted': unsorted, 'DeviceCSR': device}

    ref = ref_measure(pub.indptr, pub.indices, pub.vals, spr.Ur, spr.X_cnt[:, 0], spr.X_scl[::N_POINTS, 0], N_POINTS, 0, N)
    return spr, pub, forms, ref


def test_train_takes_the_three_forms(eng, fitted):
    spr, pub, forms, ref = fitted
    assert spr.Ur.shape == (N, 5) and spr.X_scl[::N_POINTS, 0].shape == (N_FEATURES,)
    thetas = {}
    for name, C in forms().items():
        spr.train(C)
        thetas[name] = np.array(spr.Theta)
    assert all(th.tobytes() == thetas['ndarray'].tobytes() for th in thetas.values())
    WORST['train'] = check_measure((thetas['ndarray'], np.array(eng.to_host(spr._d['cnt'])), None), ref, 'train')
    print(f"train: worst error / bar = {WORST['train']:.3f}")


def test_unscale_data_with_sampling(eng, fitted):
    """x = (C X_scl) x0 + C X_cnt.  got = fl(scl' x0 + cnt') with scl', cnt' within their measure bars: the bar is
    |x0| bar_scl + bar_cnt, and two roundings of the result (the product and the sum, fused or not)"""
    spr, pub, forms, ref = fitted
    x0 = np.random.default_rng(8).standard_normal(len(pub.names)) * 10.0 ** np.arange(-3, len(pub.names) - 3)[::-1].clip(-3, 3)
    want = ref['scl'] * x0.astype(LD) + ref['cnt']
    bar = (np.abs(x0) * measure_bar(ref['L'], ref['T_scl']) + measure_bar(ref['L'], ref['T_cnt'])
           + 2 * LD(U53) * (np.abs(ref['scl'] * x0) + np.abs(ref['cnt'])))
    gots = [spr.unscale_data(x0, sampling=C) for _ in range(2) for C in forms().values()]
    assert all(g.shape == want.shape and g.tobytes() == gots[0].tobytes() for g in gots)
    err = np.abs(gots[0].astype(LD) - want)
    assert np.all(err[bar == 0] == 0) and np.all(err <= bar)
    WORST['unscale_data'] = float((err[bar > 0] / bar[bar > 0]).max(initial=0))
    print(f"unscale_data(sampling=): worst error / bar = {WORST['unscale_data']:.3f}")


def test_reconstruct_with_sampling(eng, fitted):
    """x[i, p] = (C X_scl)_i ((C Ur)_i . a_p) + (C X_cnt)_i.  The kernel works on Theta', scl', cnt' within their measure bars, so
    the bar is the reconstruct bar plus |scl_i| sum_k |a_pk| bar_Theta_ik + bar_scl_i sum_k |a_pk Theta_ik| + bar_cnt_i; the
    products of two errors are below 2^-100 of the scale and are covered by a factor 1 + 2^-40."""
    spr, pub, forms, ref = fitted
    r, n_p = 5, 3
    Ar = np.random.default_rng(9).standard_normal((n_p, r)) * np.array([[1e-2], [1.0], [30.0]])
    want, T = ref_reconstruct(ref['Theta'], Ar, ref['scl'], ref['cnt'])
    absA = np.abs(Ar).astype(LD)
    bar = (reconstruct_bar(r, T) + np.abs(ref['scl']) * (absA @ measure_bar(ref['L'], ref['T_Theta']).T)
           + measure_bar(ref['L'], ref['T_scl']) * (absA @ np.abs(ref['Theta']).T) + measure_bar(ref['L'], ref['T_cnt']))
    bar = bar * (1 + LD(2.0) ** -40)
    gots = [spr.reconstruct(Ar, sampling=C) for _ in range(2) for C in forms().values()]
    assert all(g.shape == (len(pub.names), n_p) and g.tobytes() == gots[0].tobytes() for g in gots)
    err = np.abs(gots[0].T.astype(LD) - want)
    assert np.all(err[bar == 0] == 0) and np.all(err <= bar)
    WORST['reconstruct(sampling=)'] = float((err[bar > 0] / bar[bar > 0]).max(initial=0))
    print(f"reconstruct(sampling=): worst error / bar = {WORST['reconstruct(sampling=)']:.3f}")


def test_device_csr_dot(eng, fitted):
    _, pub, forms, _ = fitted
    x = np.random.default_rng(10).standard_normal(N) * 10.0 ** np.random.default_rng(11).uniform(-3, 3, N)
    ref = ref_measure(pub.indptr, pub.indices, pub.vals, None, x, SCALE, N_POINTS, 0, N)
    got = [forms()['DeviceCSR'].dot(x) for _ in range(2)]
    assert got[0].tobytes() == got[1].tobytes()
    WORST['DeviceCSR.dot'] = check_measure((None, got[0], None), ref, 'DeviceCSR.dot')
    print(f"DeviceCSR.dot: worst error / bar = {WORST['DeviceCSR.dot']:.3f}")


def test_device_csr_without_stored_entries(eng, fitted):
    """what camera.project returns when no ray meets the grid (tests/test_raycast_gpu.py::test_no_ray_meets_the_grid)"""
    spr = fitted[0]
    t = eng.torch
    s = 4
    C = DeviceCSR(eng.zeros((s + 1,), dtype=t.int64), eng.empty((0,), dtype=t.int64), eng.empty((0,)), (s, N), engine=eng)
    assert C.nnz == 0
    y = C.dot(np.arange(N, dtype=np.float64))
    assert y.shape == (s,) and y.dtype == np.float64 and not y.any()
    for form in (C, np.zeros((s, N))):                        # and a dense C of zeros
        spr.train(form)
        assert np.asarray(spr.Theta).shape == (s, 5) and not np.asarray(spr.Theta).any()
        assert not np.array(eng.to_host(spr._d['cnt'])).any()
        x = spr.unscale_data(np.ones(s), sampling=form)
        assert x.shape == (s,) and not x.any()
        xr = spr.reconstruct(np.ones((2, 5)), sampling=form)
        assert xr.shape == (s, 2) and not xr.any()


def test_zz_worst_ratio_overall():
    """the figure DESIGN.md records; runs last in this file"""
    if WORST:
        print('measure worst error / bar over all cases:', f'{max(WORST.values()):.3f}', 'in', max(WORST, key=WORST.get))
        assert max(WORST.values()) <= 1.0

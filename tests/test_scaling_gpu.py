"""Every scaling and centring of ROM.scale_data / fit on the GPU: the eleven scalings x axis_cnt in {1, -1, None}, f64 and
f32 storage, positive and signed data, against the np.longdouble restatement of the reference's lines 106-169 in
tests/test_scaling_host.py.  That file holds the data maker, the reference, the check functions (they take the engine) and,
in its module docstring, THE BARS with their derivation, written down before the first GPU run; the NumPy engine passes the
same checks there.  Every case prints its largest error as a fraction of its bar.

Which routine is under test where:
* csrc/combine.hip (the switch over the eight scale codes, Chan merge, scaled sum): scale_data and fit with axis_cnt = 1 / -1
  and a code scaling at m >= 25, every scale_data call with such a scaling at any m; gram_combine directly in test 4.
* csrc/spectrum.hip (the same switch, written a second time): fit at m = 7 and m = 24 (asserted: no fallback, no host Gram
  matrix); spectrum directly in test 4.
* ROM._feature_scale after the host's Chan merge: axis_cnt = None, and 'range' / 'max' / 'median' at any centring, with
  spr_feature_minmax_* (csrc/scale.hip) and the radix selection (csrc/select.hip) behind them.
* spr_colsums_* and spr_fill_feature_f64: axis_cnt = None (m = 600: two launches of 512 columns).
* spr_scale_rows_*, spr_unscale_f64 (scale[f] and rowscale branches): X0, unscale_data with and without a sampling matrix;
  directly, on row windows that begin and end inside features, in test 3; the blocked X0 route in test 2.
THE BARS, stated before the first GPU run (u = 2^-53, n_p = n_points, A = mean |x| of a row or block; the derivations and the
code that evaluates them are in the host file's docstring and functions -- one copy, so the two files cannot drift apart):
* X_cnt: m u A_i per row (any summation order); block mean (m + 4 (n_p + ranks)) u A_f.
* variance: relative (4 n_p + m + 8 + 6 ranks) u + 2 m u cross_f, cross_f = sum_i |mean_i - mu| A_i / (n_p var) <= max |x| / sd,
  from var = (trace G_f + m M2) / (n_p m) with row means that are themselves m u A_i off; the eight code scalings propagate it
  (std 1/2, pareto 1/4, vast + the mean's, l2-norm weighted), 'none' and 'max' are exact, 'range' and 'median' 2 u.
* X0: bar_cnt / |scl| + |X0| (rel_scl + 3 u); unscale_data 4 u (|x - cnt| + bar_cnt) + 2 u |x|; the kernels alone: scale_rows,
  fill_feature, feature_minmax exact, unscale 1 ulp of |scl x0| + |cnt|, colsums (rows + 2) u sum |terms|.
* Sigma_r: max rel_scl sigma_i + |bar_cnt / scl|_2 sqrt(m) + 3 u |X0|_F + dG / (2 sigma_i) + m u sigma_1, dG = (n + 2) u |X0|_F^2 + 4 m
  u sigma_1^2 (+ the colsums correction with axis_cnt = None) -- the Gram route's c m u sigma_1^2 / sigma_i.
* fields: per row, sin_t |x_i - cnt_i|_2 + the row's own bars, sin_t the Davis-Kahan bound on the turn of the leading subspace;
  entrywise, and below 1e-9 of the feature's largest entry.
Every bar that is not exact is asserted below 1e-9 relative (assert_small).
The shapes are the smallest at which these paths differ: (77, 7) features break inside a 64-row panel, (77, 24) / (77, 25)
either side of the all-device route, (130, 65) one column past a wave, (50, 300) the column-split Gram pass, (50, 600)."""
import numpy as np
import pytest

from openmeasure_amd.rom import ROM
from openmeasure_amd.sparse_sensing import SPR
from tests.test_scaling_host import (AXES, CASES, CODE_SCALINGS, F, IDS, SCALINGS, U, WINDOWS, assert_small, check_fit,
                                     check_kernels_on_window, check_scale_data, make_case, reference, reference_svd,
                                     spectrum_bars, worst, wrap_column_slice)

pytestmark = pytest.mark.gpu
f64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


# ------------------------------------------------------------------------------------------------ 1. scale_data
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('scale_type', SCALINGS)
@pytest.mark.parametrize('n_points,m,axis_cnt', CASES, ids=IDS)
def test_scale_data_matrix(eng, n_points, m, axis_cnt, scale_type, variant, dtype):
    """X_cnt, X_scl (signs and NaN exactly as the reference), X0, unscale_data(X0[:, j]) and unscale_data(x0, sampling=S)"""
    check_scale_data(eng, n_points, m, variant, dtype, scale_type, axis_cnt)


@pytest.mark.parametrize('scale_type', SCALINGS)
@pytest.mark.parametrize('axis_cnt', AXES)
def test_scale_data_on_a_column_slice(eng, scale_type, axis_cnt):
    """the same on a DeviceMatrix over columns [2, 2 + m) of a wider buffer (row stride m + 5, the neighbours hold 1e30)"""
    check_scale_data(eng, 130, 65, 'signed', 'f64', scale_type, axis_cnt, wrap=wrap_column_slice(eng.to_device))


# ------------------------------------------------------------------------------------------------ 2. blocked X0
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('n_points,m,scale_type,axis_cnt', [(77, 7, 'std', 1), (77, 7, 'range', None), (50, 300, 'vast', 1),
                                                            (50, 300, 'median', None)])
def test_blocked_x0_is_bit_identical(eng, monkeypatch, n_points, m, scale_type, axis_cnt, dtype):
    """X0 through device blocks of 13 rows (blocks begin inside features, the last one is short) against the unblocked X0 of the
    same object state: the arithmetic per element is the same, only the feature lookup of a block's rows can differ."""
    spr = SPR(make_case(n_points, m, 'signed', dtype), F, None, engine=eng)
    whole = spr.scale_data(scale_type, axis_cnt).copy()
    calls = []
    staged = eng._to_host_staged
    monkeypatch.setattr(eng, '_to_host_staged', lambda t, out=None: (calls.append(t.shape[0]), staged(t, out=out))[1])
    monkeypatch.setattr(ROM, '_X0_BLOCK_BYTES', 13 * 8 * m)
    spr._host.pop('X0')
    blocked = spr.X0
    n = F * n_points
    assert calls == [13] * (n // 13) + [n % 13] and n % 13                              # the blocked route was the one taken
    assert np.array_equal(blocked, whole)


# ------------------------------------------------------------------------------------------------ 3. kernels on row windows
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('n_points,m,row0,n_loc', WINDOWS)
def test_kernels_on_row_windows(eng, n_points, m, row0, n_loc, dtype):
    """scale_rows, fill_feature, feature_minmax exact; unscale (scale[f] and rowscale) to 1 ulp; colsums at its bar"""
    check_kernels_on_window(eng, n_points, m, row0, n_loc, dtype)


# ------------------------------------------------------------------------------------------------ 4. the two switches
def gram_reference(ref, n_points, m):
    """G = X0^T X0 in longdouble and its entrywise bar: per feature, over scl_f^2, (n_p + 4) u |C|^T |C| for the products and
    the sum over the rows (the ranks' partial sums included), m u sum_i A_i (|c_ij| + |c_ik|) for the row means' own error,
    (2 rel_scl + 3 u) |C|^T |C| for the scale, its square and the division; F u of the total for the sum over the features."""
    st = ref['st']
    X0 = ref['X0']
    G = X0.T @ X0
    B = np.zeros((m, m))
    tot = np.zeros((m, m))
    for f in range(F):
        C = np.abs(f64(st['x'][f] - st['rowmean'][f][:, None]))
        T = C.T @ C
        s = C.T @ f64(st['rowabs'][f])
        scl2 = float(ref['scl'][f]) ** 2
        B += ((n_points + 4) * U * T + m * U * (s[:, None] + s[None, :]) + (2 * ref['rel_scl'][f] + 3 * U) * T) / scl2
        tot += T / scl2
    return G, B + (F + 1) * U * tot


@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('scale_type', CODE_SCALINGS)
@pytest.mark.parametrize('n_points,m', [(77, 7), (77, 24), (130, 65)])
def test_the_two_switches_on_one_rank(eng, n_points, m, scale_type, variant):
    """gram_combine and (m <= 24) spectrum on the blocks and statistics of stats_gram: scale, 1 / scale and the merged
    statistics per feature against the longdouble reference, the combined G against X0^T X0, the spectrum's S against the
    singular values of X0; the two routes agree on the scale to 2 ulp."""
    ref = reference(n_points, m, variant, 'f64', scale_type, 1)
    fin, scl = ref['finite'], f64(ref['scl'])
    rowmean, fstats, gram = eng.stats_gram(eng.to_device(make_case(n_points, m, variant)), 0, n_points, F)
    routes = {}
    packed, scale_c, inv_c = eng.gram_combine(gram, fstats[None], scale_type)
    packed = eng.to_host(packed)
    routes['combine'] = (eng.to_host(scale_c), eng.to_host(inv_c), packed[m * m:].reshape(F, 5))
    r = 4 if m == 7 else 6
    if m <= 24:
        sp = eng.spectrum(gram, fstats[None], scale_type, r)
        routes['spectrum'] = (eng.to_host(sp['scale']), eng.to_host(sp['inv_scale']), eng.to_host(sp['feat']))
    out = {}
    assert_small('scl', ref['rel_scl'])
    assert_small('mean', ref['bar_mu'] / f64(ref['st']['A']))
    assert_small('var', ref['rel_var'])
    for name, (s, inv, feat) in routes.items():
        assert np.array_equal(np.isnan(s), ~fin) and np.array_equal(np.isnan(inv), ~fin), (name, s)
        assert np.array_equal(np.signbit(s[fin]), np.signbit(scl[fin])) and np.array_equal(feat[:, 3], s, equal_nan=True)
        out[name + ' scale'] = worst(np.abs(s[fin] - ref['scl'][fin]), ref['rel_scl'][fin] * np.abs(scl[fin]))
        out[name + ' 1/scale'] = worst(np.abs(inv[fin] - 1 / ref['scl'][fin]), (ref['rel_scl'][fin] + 2 * U) / np.abs(scl[fin]))
        assert np.array_equal(feat[:, 0], np.full(F, float(n_points)))
        out[name + ' mean'] = worst(np.abs(feat[:, 1] - ref['st']['mean']), ref['bar_mu'])
        out[name + ' var'] = worst(np.abs(feat[:, 2] - ref['st']['var']), ref['rel_var'] * f64(ref['st']['var']))
    if 'spectrum' in routes:
        a, b = routes['combine'][0][fin], routes['spectrum'][0][fin]
        assert np.all(np.abs(a - b) <= 4 * U * np.abs(a)), (a, b)                        # 2 ulp
    if fin.all():
        G, B = gram_reference(ref, n_points, m)
        assert_small('G', np.max(B) / np.max(np.abs(f64(G))))
        out['G'] = worst(np.abs(packed[:m * m].reshape(m, m) - G), B)
        if 'spectrum' in routes:
            _, _, S, Vt = reference_svd(n_points, m, variant, 'f64', scale_type, 1)
            dG, bar_S, _ = spectrum_bars(ref, S, Vt, n_points, m, 1, r)
            assert_small('S', bar_S / S[:r])
            out['S'] = worst(np.abs(eng.to_host(sp['S'])[:r] - S[:r]), bar_S)
            info = eng.to_host(sp['info'])                                               # sweeps, off^2, diag^2: fit()'s own verdict
            assert info[0] < eng.spectrum_max_sweeps or info[1] <= 1e-24 * info[2], info
    else:
        assert np.isnan(packed[:m * m]).all()
    print(f'switches {n_points}x{m} {variant} {scale_type}: error / bar ' + ' '.join(f'{k} {v:.3f}' for k, v in out.items()))


@pytest.mark.parametrize('scale_type', CODE_SCALINGS)
@pytest.mark.parametrize('m', [7, 24])
def test_the_two_switches_on_three_ranks(eng, m, scale_type):
    """fstats_all of three row windows of a global matrix with FIVE features, the Gram blocks summed: global feature 2 has no
    rows anywhere, the middle rank none of feature 0.  The merged mean / variance / scale of the four present features are
    those of the whole matrix, the absent feature has count 0, scale 1 and adds nothing to G."""
    n_points, Fg, present = 77, 5, [0, 1, 3, 4]
    ref = reference(n_points, m, 'positive', 'f64', scale_type, 1, ranks=3)
    X = make_case(n_points, m, 'positive')
    Xg = np.zeros((Fg * n_points, m))
    for k, f in enumerate(present):
        Xg[f * n_points:(f + 1) * n_points] = X[k * n_points:(k + 1) * n_points]
    gram, fs = None, []
    for row0, row1 in [(0, 121), (121, 2 * n_points), (3 * n_points, 5 * n_points)]:
        _, fstats, g = eng.stats_gram(eng.to_device(Xg[row0:row1]), row0, n_points, Fg)
        fs.append(fstats)
        gram = g if gram is None else gram + g
    fs_all = eng.torch.stack(fs)
    counts = eng.to_host(fs_all)[:, :, 0]
    assert np.array_equal(counts, [[77, 44, 0, 0, 0], [0, 33, 0, 0, 0], [0, 0, 0, 77, 77]])
    packed, scale_c, inv_c = eng.gram_combine(gram, fs_all, scale_type)
    packed = eng.to_host(packed)
    r = 4 if m == 7 else 6
    sp = eng.spectrum(gram, fs_all, scale_type, r)
    out = {}
    assert_small('scl', ref['rel_scl'])
    assert_small('mean', ref['bar_mu'] / f64(ref['st']['A']))
    assert_small('var', ref['rel_var'])
    a, b = eng.to_host(scale_c), eng.to_host(sp['scale'])
    assert np.all(np.abs(a - b) <= 4 * U * np.abs(a)), (a, b)                            # the two routes agree to 2 ulp
    for name, s, inv, feat in (('combine', eng.to_host(scale_c), eng.to_host(inv_c), packed[m * m:].reshape(Fg, 5)),
                               ('spectrum', eng.to_host(sp['scale']), eng.to_host(sp['inv_scale']), eng.to_host(sp['feat']))):
        assert s[2] == 1.0 and inv[2] == 1.0 and np.array_equal(feat[2], [0.0, 0.0, 0.0, 1.0, 0.0]), (name, s, feat)
        assert np.array_equal(feat[present, 0], np.full(F, float(n_points)))
        out[name + ' scale'] = worst(np.abs(s[present] - ref['scl']), ref['rel_scl'] * np.abs(f64(ref['scl'])))
        out[name + ' 1/scale'] = worst(np.abs(inv[present] - 1 / ref['scl']), (ref['rel_scl'] + 2 * U) / np.abs(f64(ref['scl'])))
        out[name + ' mean'] = worst(np.abs(feat[present, 1] - ref['st']['mean']), ref['bar_mu'])
        out[name + ' var'] = worst(np.abs(feat[present, 2] - ref['st']['var']), ref['rel_var'] * f64(ref['st']['var']))
    G, B = gram_reference(ref, n_points, m)
    out['G'] = worst(np.abs(packed[:m * m].reshape(m, m) - G), B)
    assert_small('G', np.max(B) / np.max(np.abs(f64(G))))
    _, _, S, Vt = reference_svd(n_points, m, 'positive', 'f64', scale_type, 1)
    dG, bar_S, _ = spectrum_bars(ref, S, Vt, n_points, m, 1, r)
    assert_small('S', bar_S / S[:r])
    out['S'] = worst(np.abs(eng.to_host(sp['S'])[:r] - S[:r]), bar_S)
    print(f'switches on three ranks 77x{m} {scale_type}: error / bar ' + ' '.join(f'{k} {v:.3f}' for k, v in out.items()))


# ------------------------------------------------------------------------------------------------ 5. fit
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('variant', ['positive', 'signed'])
@pytest.mark.parametrize('scale_type', SCALINGS)
@pytest.mark.parametrize('n_points,m,axis_cnt', CASES, ids=IDS)
def test_fit_per_combination(eng, n_points, m, axis_cnt, scale_type, variant, dtype):
    """Sigma_r and the first three training snapshots, reconstructed, at their bars; LinAlgError for the signed 'poisson'.
    At m <= 24 with row centring and a code scaling the all-device route must have been the one taken (the data meet its
    conditions with a factor 4 to spare: test_the_data_stays_on_the_all_device_route of the host file)."""
    spr, out = check_fit(eng, n_points, m, variant, dtype, scale_type, axis_cnt)
    if out and m <= 24 and axis_cnt is not None and scale_type in CODE_SCALINGS:
        assert not getattr(spr, '_device_fit_fallback_', False) and '_G' not in spr.__dict__
        assert spr.gram_refine_passes_ == 0 and spr.precentered_ is False

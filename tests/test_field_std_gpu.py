"""ROM.reconstruct_std on the HIP engine: the diagonal-form and factor-form kernels (csrc/field_std.hip) against np.longdouble
NumPy on the same inputs, at the smallest shapes where they can go wrong, one long block, the public methods end to end and
a plain-C caller.

Bar (derived in tests/test_field_std_host.py, whose variance_bar computes it, here in longdouble): per row and vector
    |out^2 - s^2 v| <= s^2 (sum_t (2 |p_t| e_t + e_t^2) + gamma_{q+2} v) + 8 2^-53 s^2 v,
p_t = sum_c u_c L_ct,  e_t = gamma_{r+2} sum_c |u_c L_ct|,  v = sum_t p_t^2;  the diagonal form is L = diag(S), q = r.  No
slack factor.  An f32-stored basis is widened on the NumPy side as on the device: the same bar.

Layouts: features of 333 cells; blocks of 1, 63, 64 and 65 rows from row 0 of F = 3, the whole 999 rows, 1000 rows (with a
fourth feature that holds the one row past 999: a short last segment), and 700 rows from row0 = 200 (starts inside feature
0, ends inside feature 2) -- so segment boundaries fall inside 64-row panels.
The long block (238 909 rows, r = q = 64, k = 16) would take the longdouble products a minute: 3 000 of its rows (both ends,
both sides of every segment boundary, a random sample) are held to the bar in longdouble, and ALL rows to twice the bar
against the f64 products of the same formula (two computed values, each within the bar of the exact one)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_field_std_host import variance_bar, variance_bar_diag

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
N_POINTS = 333
# (rows, row0, n_features)
LAYOUTS = [(1, 0, 3), (63, 0, 3), (64, 0, 3), (65, 0, 3), (999, 0, 3), (1000, 0, 4), (700, 200, 3)]


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _basis(eng, n, r, f32, pad, seed):
    import torch
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n, r)) / np.sqrt(r)
    if f32:
        U = U.astype(np.float32)
    buf = np.zeros((n, r + pad), dtype=U.dtype)
    buf[:, :r] = U
    t = eng.to_device(buf, dtype=torch.float32 if f32 else torch.float64)[:, :r]
    assert t.stride(0) == r + pad
    return t, U.astype(np.float64)


def _row_scale(n, row0, n_points, scale, rowscale):
    feat = np.minimum((row0 + np.arange(n)) // n_points, len(scale) - 1)
    return scale[feat] if rowscale is None else rowscale


def _check(out, U, L, s, tag, rows=None, S=None):
    """out (k, n) against the longdouble variance at the bar of the module docstring; S: the diagonal form, L = diag(S)"""
    if rows is not None:
        out, U, s = out[:, rows], U[rows], s[rows]
    want, bar = variance_bar(U, L, s, dtype=LD) if S is None else variance_bar_diag(U, S, s, dtype=LD)
    err = np.abs(out.astype(LD) ** 2 - want)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0)).astype(np.float64)
    print('field_std', tag, 'worst error / bar', ratio.max() if ratio.size else 0.0)
    assert np.all(err <= bar), (tag, ratio.max())


def _run(eng, Ud, row0, n_points, F, scale, S=None, L=None, rowscale=None, wide_out=False):
    """-> host (k, n); wide_out: written into a column slice of a wider buffer whose other columns must stay untouched"""
    k, n = (len(S) if S is not None else len(L)), Ud.shape[0]
    kw = dict(S=None if S is None else eng.to_device(S), L=None if L is None else eng.to_device(L),
              rowscale=None if rowscale is None else eng.to_device(rowscale))
    args = (Ud, row0, n_points, F, eng.to_device(scale))
    if not wide_out:
        out = eng.to_host(eng.field_std(*args, **kw))
    else:
        buf = eng.empty((k, n + 11))
        buf.fill_(-7.5)
        res = eng.field_std(*args, out=buf[:, 5:5 + n], **kw)
        assert res.data_ptr() == buf[:, 5:].data_ptr()
        host = eng.to_host(buf)
        assert np.all(host[:, :5] == -7.5) and np.all(host[:, 5 + n:] == -7.5)
        out = np.ascontiguousarray(host[:, 5:5 + n])
    again = eng.to_host(eng.field_std(*args, **kw))
    assert out.shape == (k, n) and out.dtype == np.float64
    assert np.array_equal(out, again)                              # no atomics: two runs are bit-identical
    return out


# ---------------------------------------------------------------------------------------------------- diagonal form
@pytest.mark.parametrize('f32', [False, True], ids=['u64', 'u32'])
@pytest.mark.parametrize('r', [1, 5, 16, 17, 64, 128, 130])
def test_diag_grid(eng, r, f32):
    rng = np.random.default_rng(100 + r)
    scale = rng.uniform(0.5, 2.0, 4)
    for n, row0, F in LAYOUTS:
        Ud, U = _basis(eng, n, r, f32, 0, seed=r * 1000 + n)
        s = _row_scale(n, row0, N_POINTS, scale[:F], None)
        for k in (1, 16, 17, 40):
            S = rng.standard_normal((k, r))
            out = _run(eng, Ud, row0, N_POINTS, F, scale[:F], S=S)
            _check(out, U, None, s, ('diag', r, f32, n, row0, k), S=S)


@pytest.mark.parametrize('f32', [False, True], ids=['u64', 'u32'])
@pytest.mark.parametrize('r,pad', [(5, 3), (17, 1), (64, 6), (130, 2)])
def test_diag_padded_basis_sliced_out_and_rowscale(eng, r, pad, f32):
    rng = np.random.default_rng(200 + r)
    scale = rng.uniform(0.5, 2.0, 3)
    n, row0, F = 700, 200, 3
    Ud, U = _basis(eng, n, r, f32, pad, seed=r)
    S = rng.standard_normal((17, r))
    out = _run(eng, Ud, row0, N_POINTS, F, scale, S=S, wide_out=True)
    _check(out, U, None, _row_scale(n, row0, N_POINTS, scale, None), ('diag padded', r, f32), S=S)
    rowscale = rng.uniform(0.1, 3.0, n)
    out = _run(eng, Ud, row0, N_POINTS, F, scale, S=S, rowscale=rowscale, wide_out=True)
    _check(out, U, None, rowscale, ('diag rowscale', r, f32), S=S)


# ---------------------------------------------------------------------------------------------------- factor form
FACTOR_RQ = [(r, q) for r in (5, 16, 17, 64, 128) for q in sorted({1, 3, 16, 17, 64, r}) if q <= r]


@pytest.mark.parametrize('k', [1, 3, 17])
@pytest.mark.parametrize('r,q', FACTOR_RQ)
def test_factor_grid(eng, r, q, k):
    rng = np.random.default_rng(300 + 7 * r + q + k)
    scale = rng.uniform(0.5, 2.0, 4)
    L = rng.standard_normal((k, r, q)) / np.sqrt(q)
    for n, row0, F in LAYOUTS:
        Ud, U = _basis(eng, n, r, False, 0, seed=r * 1000 + n + 1)
        out = _run(eng, Ud, row0, N_POINTS, F, scale[:F], L=L)
        _check(out, U, L, _row_scale(n, row0, N_POINTS, scale[:F], None), ('factor', r, q, k, n, row0))


@pytest.mark.parametrize('f32', [False, True], ids=['u64', 'u32'])
@pytest.mark.parametrize('r,q,pad', [(5, 3, 3), (17, 17, 1), (64, 33, 6), (128, 128, 2), (100, 40, 0)])
def test_factor_padded_basis_sliced_out_and_rowscale(eng, r, q, pad, f32):
    rng = np.random.default_rng(400 + r)
    scale = rng.uniform(0.5, 2.0, 3)
    n, row0, F = 700, 200, 3
    Ud, U = _basis(eng, n, r, f32, pad, seed=r + 1)
    L = rng.standard_normal((3, r, q)) / np.sqrt(q)
    out = _run(eng, Ud, row0, N_POINTS, F, scale, L=L, wide_out=True)
    _check(out, U, L, _row_scale(n, row0, N_POINTS, scale, None), ('factor padded', r, q, f32))
    rowscale = rng.uniform(0.1, 3.0, n)
    out = _run(eng, Ud, row0, N_POINTS, F, scale, L=L, rowscale=rowscale, wide_out=True)
    _check(out, U, L, rowscale, ('factor rowscale', r, q, f32))


def test_refusals(eng):
    Ud, _ = _basis(eng, 65, 129, False, 0, seed=1)
    sc = eng.to_device(np.ones(3))
    with pytest.raises(ValueError):                                # the factor form takes r <= 128: refused in Python ...
        eng.field_std(Ud, 0, N_POINTS, 3, sc, L=eng.to_device(np.ones((1, 129, 2))))
    out = eng.empty((1, 65))
    rc = eng.lib.spr_field_std_factor_f64(Ud.data_ptr(), 65, 129, 129, 0, N_POINTS, 3, sc.data_ptr(), None,
                                          eng.to_device(np.ones((1, 129, 2))).data_ptr(), 1, 2, out.data_ptr(), 65, None)
    assert rc == -1 and b'129' in eng.lib.spr_last_error()         # ... and by the library: SPR_E_INVALID
    U8, _ = _basis(eng, 65, 8, False, 0, seed=2)
    for kw in (dict(), dict(S=eng.to_device(np.ones((1, 8))), L=eng.to_device(np.ones((1, 8, 2)))),
               dict(S=eng.to_device(np.ones((1, 7)))), dict(L=eng.to_device(np.ones((1, 8, 9)))),
               dict(L=eng.to_device(np.ones((1, 7, 2)))), dict(S=eng.to_device(np.ones((2, 8))), out=eng.empty((1, 65)))):
        with pytest.raises(ValueError):
            eng.field_std(U8, 0, N_POINTS, 3, sc, **kw)
    with pytest.raises(ValueError):                                # the block does not fit the feature layout
        eng.field_std(U8, 990, N_POINTS, 3, sc, S=eng.to_device(np.ones((1, 8))))
    assert eng.lib.spr_field_std_factor_f64(U8.data_ptr(), 65, 8, 8, 0, N_POINTS, 3, sc.data_ptr(), None,
                                            eng.to_device(np.ones((1, 8, 2))).data_ptr(), 1, 2, out.data_ptr(), 64, None) == -1


# ---------------------------------------------------------------------------------------------------- further cases
def test_long_block_both_forms(eng):
    """features of 100 003 cells, a block of 238 909 rows that starts inside feature 1 of 4 and ends inside feature 3:
    every workgroup runs its steady-state panel loop"""
    n_points, F, r, q, k = 100_003, 4, 64, 64, 16
    row0, n = n_points + 33_217, 2 * n_points + 38_903
    rng = np.random.default_rng(77)
    scale = rng.uniform(0.5, 2.0, F)
    Ud, U = _basis(eng, n, r, False, 0, seed=78)
    s = _row_scale(n, row0, n_points, scale, None)
    cuts = [g * n_points - row0 for g in range(1, F) if 0 < g * n_points - row0 < n]
    rows = np.unique(np.clip(np.concatenate([np.arange(256), n - 1 - np.arange(256)] +
                                            [c + np.arange(-130, 130) for c in cuts] +
                                            [rng.integers(0, n, 2000)]), 0, n - 1))
    S = rng.standard_normal((k, r))
    L = rng.standard_normal((k, r, q)) / np.sqrt(q)
    for tag, kw in (('diag', dict(S=S)), ('factor', dict(L=L))):
        out = _run(eng, Ud, row0, n_points, F, scale, **kw)
        _check(out, U, L, s, ('long', tag), rows=rows, S=S if tag == 'diag' else None)
        want64, bar64 = variance_bar_diag(U, S, s) if tag == 'diag' else variance_bar(U, L, s)
        assert np.all(np.abs(out ** 2 - want64) <= 2 * bar64), tag


def test_zero_rows_and_nan_vectors(eng):
    rng = np.random.default_rng(5)
    n, r, k, q = 700, 17, 5, 6
    Ud, U = _basis(eng, n, r, False, 0, seed=9)
    zero = [0, 63, 64, 333 - 200, 699]
    U[zero] = 0.0
    Ud[zero] = 0.0                                                 # as optimal_placement(mask=...) leaves masked rows
    scale = rng.uniform(0.5, 2.0, 3)
    S = rng.standard_normal((k, r))
    L = rng.standard_normal((k, r, q))
    for kw in (dict(S=S), dict(L=L)):
        out = _run(eng, Ud, 200, N_POINTS, 3, scale, **kw)
        assert np.all(out[:, zero] == 0.0) and not np.signbit(out[:, zero]).any()
        assert np.all(np.isfinite(out)) and np.all(np.delete(out, zero, axis=1) > 0)
    Sn, Ln = S.copy(), L.copy()
    Sn[2] = np.nan
    Ln[2] = np.nan
    for kw, clean in ((dict(S=Sn), dict(S=S)), (dict(L=Ln), dict(L=L))):
        out = _run_nan(eng, Ud, scale, **kw)
        ref = _run(eng, Ud, 200, N_POINTS, 3, scale, **clean)
        assert np.all(np.isnan(out[2]))
        keep = [0, 1, 3, 4]
        assert np.array_equal(out[keep], ref[keep])                # the neighbours: finite, the same bits
    # a single NaN entry poisons its vector only
    Sn = S.copy()
    Sn[1, 4] = np.nan
    out = _run_nan(eng, Ud, scale, S=Sn)
    assert np.all(np.isfinite(out[[0, 2, 3, 4]]))
    nz = np.flatnonzero(U[:, 4] != 0)
    assert np.all(np.isnan(out[1, nz]))


def _run_nan(eng, Ud, scale, **kw):
    kw = {key: eng.to_device(v) for key, v in kw.items()}
    return eng.to_host(eng.field_std(Ud, 200, N_POINTS, 3, eng.to_device(scale), **kw))


@pytest.mark.parametrize('basis', ['f64', 'f32'])
def test_public_methods_end_to_end(eng, basis):
    """fit -> optimal_placement -> train -> predict and coefficient_covariance with non-zero uncertainties, then
    reconstruct_std(cov=...) against the host formula on the downloaded Ur at the bar, and reconstruct_std(sigma=Ar_sigma)"""
    from openmeasure_amd.rom import ROM, DeviceMatrix
    from openmeasure_amd.sparse_sensing import SPR
    from openmeasure_amd.synth import make_R
    n_points, F, m, r = 1531, 3, 24, 8
    t = eng.torch
    dt = t.float32 if basis == 'f32' else t.float64
    R = eng.to_device(make_R(m, r, seed=7))
    Xd = eng.synth(n_points * F, m, 0, n_points, R, 1e-3, 7, dtype=dt)
    spr = SPR(DeviceMatrix(Xd, basis=basis), F, None, engine=eng)
    spr.fit(select_modes='number', n_modes=r)
    C = spr.optimal_placement()
    spr.train(C)
    X = eng.to_host(Xd).astype(np.float64)
    piv = spr.sensors_
    rng = np.random.default_rng(3)
    ys = []
    for j in range(3):
        y = np.zeros((len(piv), 3))
        y[:, 1] = 0.01 * (1 + np.arange(len(piv)) % 3) * (j + 1)
        y[:, 0] = X[piv, j] + y[:, 1] * rng.standard_normal(len(piv))
        y[:, 2] = piv // n_points
        ys.append(y)
    Ar, Ar_sigma = spr.predict(ys)
    cov = spr.coefficient_covariance(ys)
    assert cov.shape == (3, r, r)
    for j, y in enumerate(ys):                                     # the formula, on the object's host Theta
        sig0 = y[:, 1] / spr._scl_f[y[:, 2].astype(int)]
        P = np.linalg.pinv(np.diag(1 / sig0) @ spr.Theta)
        np.testing.assert_allclose(cov[j], P @ P.T, rtol=1e-12, atol=1e-12 * np.abs(cov[j]).max())
    U = np.asarray(spr.Ur).astype(np.float64)
    assert np.asarray(spr.Ur).dtype == (np.float32 if basis == 'f32' else np.float64)
    s = np.asarray(spr.X_scl)[:, 0]
    out = spr.reconstruct_std(cov=cov)
    assert out.shape == (n_points * F, 3) and out.dtype == np.float64 and isinstance(out, np.ndarray)
    L = ROM._cov_factors(cov)                                      # the factors the method hands to the kernel
    _check(out.T, U, L, s, ('end to end cov', basis))
    # ... and against the dense formula diag(D Ur cov Ur^T D): the bar plus the eigh slack derived in the host test
    from tests.test_field_std_host import cov_slack
    _, bar = variance_bar(U, L, s)
    sU = s[:, None] * U
    dense = np.stack([np.einsum('ic,cd,id->i', sU, c, sU) for c in cov])
    assert np.all(np.abs(out.T ** 2 - dense) <= 2 * bar + cov_slack(U, s, cov))
    dev = spr.reconstruct_std(cov=cov, to_host=False)
    assert tuple(dev.shape) == (3, n_points * F) and dev.is_cuda
    np.testing.assert_array_equal(eng.to_host(dev).T, out)
    o2 = spr.reconstruct_std(Ar_sigma)
    _check(o2.T, U, None, s, ('end to end sigma', basis), S=Ar_sigma)
    np.testing.assert_array_equal(spr.reconstruct_std(factor=L), out)


# A caller with no Python and no torch in the process: spr_field_std_diag_f64 on hipMalloc'ed memory against loops on the
# host, at the bar of the module docstring for L = diag(S): (3 g + g^2) v + 8 eps v, g = gamma_{r+2}, sums in long double.
C_SRC = r'''
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <hip/hip_runtime_api.h>
#include "spr_hip.h"
#define CK(x) do { if ((x) != 0) { printf("fail %s line %d: %s\n", #x, __LINE__, spr_last_error()); return 1; } } while (0)
int main(void) {
  const int64_t n_points = 2048, row0 = 1000, n = 4999, ldo = 5003; const int F = 3, r = 6, k = 3, ldu = 8;
  double *U = (double *)malloc(sizeof(double) * n * ldu), *out = (double *)malloc(sizeof(double) * k * ldo);
  double sc[3] = {2.0, 0.5, 1.25}, S[18];
  uint64_t s = 4242;
  for (int64_t i = 0; i < n * ldu; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; U[i] = (double)(s >> 11) / 9007199254740992.0 - 0.5; }
  for (int i = 0; i < 18; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; S[i] = (double)(s >> 11) / 9007199254740992.0 * 3.0 - 1.0; }
  if (spr_field_std_diag_f64(NULL, n, r, ldu, row0, n_points, F, NULL, NULL, NULL, k, NULL, ldo, NULL) != SPR_E_INVALID) return 2;
  double *dU, *dS, *dsc, *dout;
  CK(hipMalloc((void **)&dU, sizeof(double) * n * ldu)); CK(hipMalloc((void **)&dS, sizeof(S)));
  CK(hipMalloc((void **)&dsc, sizeof(sc))); CK(hipMalloc((void **)&dout, sizeof(double) * k * ldo));
  if (spr_field_std_diag_f64(dU, n, r, ldu, row0, n_points, F, dsc, NULL, dS, k, dout, n - 1, NULL) != SPR_E_INVALID) return 3;
  CK(hipMemcpy(dU, U, sizeof(double) * n * ldu, hipMemcpyHostToDevice)); CK(hipMemcpy(dS, S, sizeof(S), hipMemcpyHostToDevice));
  CK(hipMemcpy(dsc, sc, sizeof(sc), hipMemcpyHostToDevice));
  CK(spr_field_std_diag_f64(dU, n, r, ldu, row0, n_points, F, dsc, NULL, dS, k, dout, ldo, NULL));
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out, dout, sizeof(double) * k * ldo, hipMemcpyDeviceToHost));
  const long double eps = 0x1p-53L, g = (r + 2) * eps / (1.0L - (r + 2) * eps);
  double worst = 0.0;
  for (int j = 0; j < k; ++j)
    for (int64_t i = 0; i < n; ++i) {
      long double v = 0.0L;
      for (int c = 0; c < r; ++c) { const long double p = (long double)U[i * ldu + c] * S[j * r + c]; v += p * p; }
      const long double s2 = (long double)sc[(row0 + i) / n_points] * sc[(row0 + i) / n_points];
      const long double o = out[j * ldo + i], bar = s2 * v * (3 * g + g * g + 8 * eps);
      const double qn = (double)(fabsl(o * o - s2 * v) / bar);
      if (qn > worst) worst = qn;
    }
  if (worst > 1.0) { printf("field_std mismatch: error / bar = %g\n", worst); return 4; }
  printf("C field_std ok: worst error / bar %.3g\n", worst);
  return 0;
}
'''


def test_plain_c_caller_of_field_std_diag(tmp_path):
    assert shutil.which('gcc') is not None and os.path.exists('/opt/rocm/include/hip/hip_runtime_api.h')
    lib = os.path.join(ROOT, 'openmeasure_amd', 'libspr_hip.so')
    src = tmp_path / 'f.c'
    src.write_text(C_SRC)
    exe = tmp_path / 'f'
    subprocess.run(['gcc', '-std=gnu99', '-D__HIP_PLATFORM_AMD__', '-I', os.path.join(ROOT, 'include'),
                    '-I', '/opt/rocm/include', str(src), '-o', str(exe), lib, '-L/opt/rocm/lib', '-lamdhip64', '-lm',
                    '-Wl,-rpath,' + os.path.dirname(lib), '-Wl,-rpath,/opt/rocm/lib'], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert 'C field_std ok' in out.stdout

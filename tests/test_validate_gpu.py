"""ROM.transform / ROM.reconstruction_error on the HIP engine: the encode and field-error kernels (csrc/validate.hip) against
NumPy at the smallest shapes where they can go wrong -- the block of tests/test_cols_gpu._sweep_case (2 863 rows that start
inside feature 1 of 4 and end inside feature 3, no length a multiple of 64) -- one long block (several panels per workgroup),
the public methods end to end, and a plain-C caller.

Bars (derived in tests/test_validate_host.py, whose functions compute them): the reference is accumulated in np.longdouble;
 * encode: an entry within  gamma sum_i |Ur[i, c] x0[i, j]|,  gamma = (n + r + 4) 2^-53 -- the worst case of ANY summation
   order, four orders of magnitude below what a misplaced tile produces;
 * field error: per row |delta_i| <= (r + 6) 2^-53 (|X_cnt_i| + |X_true_ij| + X_scl sum_c |Ur[i, c] a_c|);  sse within
   2 sqrt(sse) |delta|_2 + |delta|_2^2 + gamma sse,  ss_true within gamma ss_true,  max_abs within max delta;  max_row EXACT:
   the NumPy side asserts that, per (vector, feature), the largest |d| leads the runner-up by more than 2 max delta.
f32-stored inputs are widened to f64 on the NumPy side as on the device: the same bars.
The long block (238 909 rows) would take the longdouble matrix products ten seconds; there the row products are f64 BLAS
over 512-row chunks and only the accumulation across chunks / rows is longdouble, and the encode bar is TIGHTENED by the
reference's own worst case (512 2^-53 of the same sum), never widened."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_validate_host import EPS, error_bars, numpy_encode, numpy_field_error

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _padded(eng, a, pad, f32):
    import torch
    buf = np.zeros((a.shape[0], a.shape[1] + pad), dtype=a.dtype)
    buf[:, :a.shape[1]] = a
    t = eng.to_device(buf, dtype=torch.float32 if f32 else torch.float64)[:, :a.shape[1]]
    assert t.stride(0) == a.shape[1] + pad
    return t


def _case(eng, r, k, store, seed, ldu_pad=0, ldx_pad=0, long=False):
    """store = (basis, X) storage, each 'f64' | 'f32'.  The block starts inside feature 1 of 4 and ends inside feature 3."""
    rng = np.random.default_rng(seed)
    if long:
        n_points, F = 100_003, 4
        row0, n = n_points + 33_217, 2 * n_points + 38_903
    else:
        n_points, F = 1237, 4
        row0, n = 1237 + 411, 2 * 1237 + 389
    U = rng.standard_normal((n, r)) / np.sqrt(r)
    if store[0] == 'f32':
        U = U.astype(np.float32)
    mu = rng.standard_normal(n) * 0.3
    scale = rng.uniform(0.5, 2.0, F)
    A = rng.standard_normal((k, r))
    feat = np.minimum((row0 + np.arange(n)) // n_points, F - 1)
    # a field near the reconstruction: d is a small difference of large values
    X = (U.astype(np.float64) @ A.T) * scale[feat][:, None] + mu[:, None] + 0.05 * rng.standard_normal((n, k))
    if store[1] == 'f32':
        X = X.astype(np.float32)
    return dict(Ud=_padded(eng, U, ldu_pad, store[0] == 'f32'), Xd=_padded(eng, X, ldx_pad, store[1] == 'f32'),
                U=U.astype(np.float64), X=X.astype(np.float64), mu=mu, scale=scale, A=A, row0=row0, n=n, n_points=n_points,
                F=F, r=r, k=k, long=long)


def _encode_reference(c):
    """-> (reference (k, r) longdouble, S, bar)"""
    n, r = c['n'], c['r']
    gamma = (n + r + 4) * EPS
    if not c['long']:
        ref, S = numpy_encode(c['U'], c['row0'], c['n_points'], c['F'], c['mu'], c['scale'], c['X'], dtype=LD)
        return ref, gamma * S.astype(np.float64)
    feat = np.minimum((c['row0'] + np.arange(n)) // c['n_points'], c['F'] - 1)
    x0 = (c['X'] - c['mu'][:, None]) / c['scale'][feat][:, None]
    ref = np.zeros((c['k'], r), dtype=LD)
    for i0 in range(0, n, 512):                                # f64 BLAS over 512 rows: within 512 eps S_chunk of exact
        ref += x0[i0:i0 + 512].T @ c['U'][i0:i0 + 512]
    S = np.abs(x0).T @ np.abs(c['U'])
    return ref, (gamma - 512 * EPS) * S


def _check_encode(eng, c, tag):
    args = (c['Ud'], c['row0'], c['n_points'], c['F'], eng.to_device(c['mu']), eng.to_device(c['scale']), c['Xd'])
    out = eng.to_host(eng.encode(*args))
    again = eng.to_host(eng.encode(*args))
    assert out.shape == (c['k'], c['r']) and out.dtype == np.float64
    assert np.array_equal(out, again)                             # no atomics: two runs are bit-identical
    ref, bar = _encode_reference(c)
    err = np.abs((out.astype(LD) - ref).astype(np.float64))
    print('encode', tag, 'worst error / bar', (err / bar).max())
    assert np.all(err <= bar), (tag, (err / bar).max())


def _check_field_error(eng, c, tag):
    args = (c['Ud'], c['row0'], c['n_points'], c['F'], eng.to_device(c['mu']), eng.to_device(c['scale']),
            eng.to_device(c['A']), c['Xd'])
    out = eng.to_host(eng.field_error(*args))
    again = eng.to_host(eng.field_error(*args))
    k, F, n, r = c['k'], c['F'], c['n'], c['r']
    assert out.shape == (k, F, 4)
    assert np.array_equal(out, again)
    # long block: the row products in f64 (module docstring); the sums over the rows are longdouble either way
    ref = numpy_field_error(c['U'], c['row0'], c['n_points'], F, c['mu'], c['scale'], c['A'], c['X'],
                            dtype=np.float64 if c['long'] else LD)
    if c['long']:
        ref['rec'] = ref['rec'].astype(LD)
        for f in range(F):
            sel = ref['feat'] == f
            if sel.any():                                         # f64 squares (2^-53 relative each), longdouble sums
                ref['rec'][:, f, 0] = np.sum(ref['d'][sel] ** 2, axis=0, dtype=LD)
                ref['rec'][:, f, 1] = np.sum(c['X'][sel] ** 2, axis=0, dtype=LD)
    b_sse, b_sst, b_max = error_bars(ref, n - 2 if c['long'] else n, r)      # ... taken off gamma: tightened, not widened
    rec = ref['rec']
    # precondition of an exact max_row: the leader's margin over the runner-up exceeds 2 max delta, for EVERY pair
    ad = np.abs(ref['d']).astype(np.float64)
    worst_margin = np.inf
    for f in range(F):
        sel = ref['feat'] == f
        if not sel.any():
            assert np.all(out[:, f, 3] == -1) and np.all(out[:, f, :3] == 0)      # feature 0: no row in this block
            continue
        top = np.partition(ad[sel], -2, axis=0)[-2:]
        margin = (top[1] - top[0]) / (2 * b_max[:, f])
        worst_margin = min(worst_margin, margin.min())
        assert np.all(margin > 1.0), (tag, f, margin.min())
    print('field error', tag, 'smallest margin / rounding', worst_margin)
    held = rec[:, :, 3] >= 0
    assert held.sum() == k * 3
    e_sse = np.abs((out[:, :, 0].astype(LD) - rec[:, :, 0]).astype(np.float64))
    e_sst = np.abs((out[:, :, 1].astype(LD) - rec[:, :, 1]).astype(np.float64))
    e_max = np.abs((out[:, :, 2].astype(LD) - rec[:, :, 2]).astype(np.float64))
    with np.errstate(invalid='ignore', divide='ignore'):
        print('field error', tag, 'worst error / bar: sse', np.nanmax(e_sse / b_sse), 'ss_true', np.nanmax(e_sst / b_sst),
              'max_abs', np.nanmax(e_max / b_max))
    assert np.all(e_sse[held] <= b_sse[held]) and np.all(e_sst[held] <= b_sst[held]) and np.all(e_max[held] <= b_max[held])
    assert np.array_equal(out[:, :, 3], rec[:, :, 3].astype(np.float64))            # max_row: exact, every pair


F64 = ('f64', 'f64')
ALL = [F64, ('f64', 'f32'), ('f32', 'f64'), ('f32', 'f32')]
# (r, k, ldu_pad, ldx_pad): a partial MFMA tile, the 128 boundary, the wide path (r = 200), k = 1, ragged slices (100 = 64 + 36)
SHAPES = [(6, 1, 0, 0), (6, 100, 2, 3), (32, 16, 0, 0), (64, 17, 6, 3), (64, 64, 0, 0), (100, 64, 2, 0), (128, 100, 0, 3),
          (128, 1, 6, 0), (200, 16, 0, 3), (200, 100, 6, 0), (7, 17, 0, 3)]
EVERY_STORAGE = {(6, 100), (64, 17), (128, 100), (200, 16)}
CASES = [(s, st) for s in SHAPES for st in (ALL if s[:2] in EVERY_STORAGE else [F64])]


@pytest.mark.parametrize('shape,store', CASES, ids=[f'r{s[0]}-k{s[1]}-u{st[0]}-x{st[1]}' for s, st in CASES])
def test_kernels_against_numpy(eng, shape, store):
    r, k, ldu_pad, ldx_pad = shape
    c = _case(eng, r, k, store, seed=500 + r + k, ldu_pad=ldu_pad, ldx_pad=ldx_pad)
    _check_encode(eng, c, (shape, store))
    _check_field_error(eng, c, (shape, store))


@pytest.mark.parametrize('r,k', [(64, 17), (128, 64)])
def test_kernels_many_panels(eng, r, k):
    """features of 100 003 cells, a block of 238 909 rows: every workgroup runs its steady-state panel loop"""
    c = _case(eng, r, k, F64, seed=700 + r + k, long=True)
    _check_encode(eng, c, ('long', r, k))
    _check_field_error(eng, c, ('long', r, k))


def test_engine_refuses_mismatched_shapes(eng):
    c = _case(eng, 6, 3, F64, seed=1)
    mu, sc = eng.to_device(c['mu']), eng.to_device(c['scale'])
    with pytest.raises(ValueError):
        eng.encode(c['Ud'], c['row0'], c['n_points'], c['F'], mu, sc, c['Xd'][:-1])
    with pytest.raises(ValueError):
        eng.field_error(c['Ud'], c['row0'], c['n_points'], c['F'], mu, sc, eng.to_device(c['A'][:2]), c['Xd'])
    with pytest.raises(ValueError):                               # the block does not fit the feature layout
        eng.encode(c['Ud'], c['row0'], c['n_points'], 2, mu, sc, c['Xd'])


@pytest.mark.parametrize('basis', ['f64', 'f32'])
def test_public_methods_end_to_end(eng, basis):
    """fit on a small synth case, then transform / reconstruction_error against NumPy on the object's own host arrays and
    on the downloaded reconstruct(A) field"""
    from openmeasure_amd.rom import DeviceMatrix
    from openmeasure_amd.sparse_sensing import ROM
    from openmeasure_amd.synth import make_R
    n_points, F, m, r = 1531, 3, 24, 8
    t = eng.torch
    dt = t.float32 if basis == 'f32' else t.float64
    R = eng.to_device(make_R(m, r, seed=7))
    Xd = eng.synth(n_points * F, m, 0, n_points, R, 1e-3, 7, dtype=dt)
    Xt_d = eng.synth(n_points * F, m, 0, n_points, R, 1e-3, 8, dtype=dt)[:, :5]     # held out: another seed; ldx = m
    rom = ROM(DeviceMatrix(Xd, basis=basis), F, None, engine=eng)
    rom.fit(select_modes='number', n_modes=r)
    X, Xt = eng.to_host(Xd).astype(np.float64), eng.to_host(Xt_d.contiguous()).astype(np.float64)
    U = np.asarray(rom.Ur).astype(np.float64)
    assert np.asarray(rom.Ur).dtype == (np.float32 if basis == 'f32' else np.float64)
    cnt, scl = np.asarray(rom.X_cnt)[:, 0], np.asarray(rom._scl_f)
    n = U.shape[0]
    # transform(X) against Ur.T @ X0
    A = rom.transform(DeviceMatrix(Xd))
    ref, S = numpy_encode(U, 0, n_points, F, cnt, scl, X, dtype=LD)
    err = np.abs((A.astype(LD) - ref).astype(np.float64))
    bar = (n + r + 4) * EPS * S.astype(np.float64)
    print('end to end', basis, 'transform worst error / bar', (err / bar).max())
    assert A.shape == (m, r) and np.all(err <= bar)
    if basis == 'f64':                                             # orthonormal basis of the fit: these ARE the coefficients
        np.testing.assert_allclose(A, rom.Ar, rtol=0, atol=1e-9 * np.abs(rom.Ar).max())
    # host ndarray input (uploaded as stored) gives the same bits as the tensor in place
    np.testing.assert_array_equal(rom.transform(eng.to_host(Xt_d.contiguous())), rom.transform(Xt_d))
    # reconstruction_error(X_test, A) against NumPy on the host arrays and on the downloaded field
    At = rom.transform(Xt_d)
    e = rom.reconstruction_error(Xt_d, At)
    rf = numpy_field_error(U, 0, n_points, F, cnt, scl, At, Xt, dtype=LD)
    b_sse, b_sst, b_max = error_bars(rf, n, r)
    rec = rf['rec']
    assert np.all(np.abs((e['sse'].astype(LD) - rec[:, :, 0]).astype(np.float64)) <= b_sse)
    assert np.all(np.abs((e['ss_true'].astype(LD) - rec[:, :, 1]).astype(np.float64)) <= b_sst)
    assert np.all(np.abs((e['max_abs'].astype(LD) - rec[:, :, 2]).astype(np.float64)) <= b_max)
    field = rom.reconstruct(At)                                    # (n, 5) on the host: the route this method replaces
    d = field - Xt
    for f in range(F):
        blk = slice(f * n_points, (f + 1) * n_points)
        assert np.all(np.abs((d[blk].astype(LD) ** 2).sum(axis=0).astype(np.float64) - e['sse'][:, f]) <= 2 * b_sse[:, f])
        assert np.all(np.abs(np.abs(d[blk]).max(axis=0) - e['max_abs'][:, f]) <= 2 * b_max[:, f])
        for j, row in enumerate(e['max_row'][:, f]):
            assert f * n_points <= row < (f + 1) * n_points
            assert abs(d[row, j]) >= np.abs(d[blk, j]).max() - 2 * b_max[j, f]
    np.testing.assert_array_equal(e['rmse'], np.sqrt(e['sse'] / n_points))
    e0 = rom.reconstruction_error(Xt_d)                            # Ar=None: transform's coefficients
    for key in e:
        np.testing.assert_array_equal(e0[key], e[key])


# A caller with no Python and no torch in the process: spr_encode_f64 on hipMalloc'ed memory against loops on the host, at
# the bar of the module docstring (gamma sum |terms|, the sums formed here in long double).
C_ENCODE_SRC = r'''
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <hip/hip_runtime_api.h>
#include "spr_hip.h"
#define CK(x) do { if ((x) != 0) { printf("fail %s line %d: %s\n", #x, __LINE__, spr_last_error()); return 1; } } while (0)
int main(void) {
  const int64_t n_points = 2048, row0 = 1000, n = 4999; const int F = 3, r = 6, k = 3, ldu = 8, ldx = 5;
  double *U = (double *)malloc(sizeof(double) * n * ldu), *X = (double *)malloc(sizeof(double) * n * ldx);
  double *mu = (double *)malloc(sizeof(double) * n), sc[3] = {2.0, 0.5, 1.25}, A[18];
  uint64_t s = 4242;
  for (int64_t i = 0; i < n * ldu; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; U[i] = (double)(s >> 11) / 9007199254740992.0 - 0.5; }
  for (int64_t i = 0; i < n * ldx; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; X[i] = (double)(s >> 11) / 9007199254740992.0 * 3.0; }
  for (int64_t i = 0; i < n; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; mu[i] = (double)(s >> 11) / 9007199254740992.0 + 1.0; }
  if (spr_encode_f64(NULL, n, r, ldu, NULL, k, ldx, row0, n_points, F, NULL, NULL, NULL, NULL, 0, NULL) != SPR_E_INVALID) return 2;
  double *dU, *dX, *dmu, *dsc, *dA; void *ws;
  size_t wsb = spr_encode_workspace(r, k, F);
  if (wsb == 0) return 3;
  CK(hipMalloc((void **)&dU, sizeof(double) * n * ldu)); CK(hipMalloc((void **)&dX, sizeof(double) * n * ldx));
  CK(hipMalloc((void **)&dmu, sizeof(double) * n)); CK(hipMalloc((void **)&dsc, sizeof(sc))); CK(hipMalloc((void **)&dA, sizeof(A)));
  CK(hipMalloc(&ws, wsb));
  CK(hipMemcpy(dU, U, sizeof(double) * n * ldu, hipMemcpyHostToDevice)); CK(hipMemcpy(dX, X, sizeof(double) * n * ldx, hipMemcpyHostToDevice));
  CK(hipMemcpy(dmu, mu, sizeof(double) * n, hipMemcpyHostToDevice)); CK(hipMemcpy(dsc, sc, sizeof(sc), hipMemcpyHostToDevice));
  CK(spr_encode_f64(dU, n, r, ldu, dX, k, ldx, row0, n_points, F, dmu, dsc, dA, ws, wsb, NULL));
  CK(hipMemcpy(A, dA, sizeof(A), hipMemcpyDeviceToHost));
  double worst = 0.0;
  for (int j = 0; j < k; ++j)
    for (int c = 0; c < r; ++c) {
      long double ref = 0.0L, sum = 0.0L;
      for (int64_t i = 0; i < n; ++i) {
        const double x0 = (X[i * ldx + j] - mu[i]) / sc[(row0 + i) / n_points];
        ref += (long double)x0 * U[i * ldu + c]; sum += fabsl((long double)x0 * U[i * ldu + c]);
      }
      const double q = (double)(fabsl((long double)A[j * r + c] - ref) / ((n + r + 4) * 0x1p-53L * sum));
      if (q > worst) worst = q;
    }
  if (worst > 1.0) { printf("encode mismatch: error / bar = %g\n", worst); return 4; }
  printf("C encode ok: worst error / bar %.3g\n", worst);
  return 0;
}
'''


def test_plain_c_caller_of_encode(tmp_path):
    if shutil.which('gcc') is None or not os.path.exists('/opt/rocm/include/hip/hip_runtime_api.h'):
        pytest.skip('gcc / HIP runtime headers not available')
    lib = os.path.join(ROOT, 'openmeasure_amd', 'libspr_hip.so')
    src = tmp_path / 'e.c'
    src.write_text(C_ENCODE_SRC)
    exe = tmp_path / 'e'
    subprocess.run(['gcc', '-std=gnu99', '-D__HIP_PLATFORM_AMD__', '-I', os.path.join(ROOT, 'include'),
                    '-I', '/opt/rocm/include', str(src), '-o', str(exe), lib, '-L/opt/rocm/lib', '-lamdhip64', '-lm',
                    '-Wl,-rpath,' + os.path.dirname(lib), '-Wl,-rpath,/opt/rocm/lib'], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert 'C encode ok' in out.stdout

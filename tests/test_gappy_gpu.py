"""ROM.gappy_transform on the HIP engine: the masked normal-equations kernel (csrc/gappy.hip) against NumPy at the smallest
shapes where it can go wrong -- the block of tests/test_validate_gpu._case (2 863 rows that start inside feature 1 of 4 and
end inside feature 3, no length a multiple of 64) -- one long block (several panels per workgroup), the public method end to
end, and a plain-C caller.

Bars (derived in tests/test_gappy_host.py, whose functions compute them): the reference is accumulated in np.longdouble over
the observed rows;  an entry of H within  gamma sum_i m_i |U[i, c] U[i, d]|,  an entry of B within
gamma sum_i m_i |x0[i, j] U[i, c]|,  gamma = (n + r + 4) 2^-53 -- the worst case of ANY summation order;  nobs exact.
f32-stored inputs are widened to f64 on the NumPy side as on the device: the same bars.
The long block (238 909 rows, 10 % observed): the row products are f64 BLAS over chunks of 512 observed rows and only the
accumulation across chunks is longdouble; the bars are TIGHTENED by the reference's own worst case (512 2^-53 of the same
sums), never widened."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_gappy_host import EPS, bars_of, check_against_lstsq, numpy_gappy_normal
from tests.test_validate_gpu import _case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
MASKS = ('ones', 'random', 'zero', 'feature2', 'last_row')


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def _mask(c, kind, seed):
    n = c['n']
    if kind == 'ones':
        return np.ones(n, dtype=bool)
    if kind == 'random':
        return np.random.default_rng(seed).random(n) < 0.5
    m = np.zeros(n, dtype=bool)
    if kind == 'feature2':                                      # whole panels skipped, the segment's edges inside panels
        g = c['row0'] + np.arange(n)
        m[(g >= 2 * c['n_points']) & (g < 3 * c['n_points'])] = True
    elif kind == 'last_row':                                    # one observed row, in the last, partial panel of the block
        m[n - 1] = True
    return m


def _device_mask(eng, m, width):
    """width 1: a contiguous (n,) uint8 tensor; else column 1 of an (n, width) row-major mask whose other columns differ"""
    import torch
    if width == 1:
        return eng.to_device(m.astype(np.uint8), dtype=torch.uint8)
    full = np.repeat((~m).astype(np.uint8)[:, None], width, axis=1)
    full[:, 1] = m * 7                                          # any non-zero byte means observed
    t = eng.to_device(full, dtype=torch.uint8)[:, 1]
    assert t.stride(0) == width
    return t


def _run(eng, c, Xd, md):
    H, B, nobs = eng.gappy_normal(c['Ud'], c['row0'], c['n_points'], c['F'], c['mu_d'], c['scale_d'], Xd, md)
    assert H._base is B._base and H._base is nobs._base and H._base.numel() == c['r'] ** 2 + c['k'] * c['r'] + 1
    return eng.to_host(H._base).copy()


def _with_unobserved(eng, c, m, value):
    """the case's X with the unobserved rows overwritten, stored and padded like c['Xd']"""
    import torch
    X = eng.to_host(c['Xd'].contiguous()).copy()
    X[~m] = value
    buf = np.zeros((c['n'], c['Xd'].stride(0)), dtype=X.dtype)
    buf[:, :c['k']] = X
    return eng.to_device(buf, dtype=torch.float32 if X.dtype == np.float32 else torch.float64)[:, :c['k']]


def _check(eng, c, kind, width, tag, reference=None):
    r, k, n = c['r'], c['k'], c['n']
    m = _mask(c, kind, seed=n + r + k)
    md = _device_mask(eng, m, width)
    out = _run(eng, c, c['Xd'], md)
    H, B, nobs = out[:r * r].reshape(r, r), out[r * r:r * r + k * r].reshape(k, r), out[-1]
    assert np.array_equal(out, _run(eng, c, c['Xd'], md))          # no atomics: two runs are bit-identical
    assert np.array_equal(H, H.T)                                 # H is bit-symmetric
    assert nobs == m.sum()                                        # a count: exact
    if kind == 'zero':
        assert not out.any()                                      # exactly 0
    if kind != 'ones':                                            # unobserved entries are selected away: NaN there = 0 there, bit for bit
        o_nan = _run(eng, c, _with_unobserved(eng, c, m, np.nan), md)
        o_zero = _run(eng, c, _with_unobserved(eng, c, m, 0.0), md)
        assert np.array_equal(o_nan, o_zero) and np.array_equal(o_nan, out)
    if reference is None:
        ref = numpy_gappy_normal(c['U'], c['row0'], c['n_points'], c['F'], c['mu'], c['scale'], c['X'], m, dtype=LD)
        bH, bB = bars_of(ref, n, r)
    else:
        ref, bH, bB = reference(c, m)
    eH = np.abs((H.astype(LD) - ref['H']).astype(np.float64))
    eB = np.abs((B.astype(LD) - ref['B']).astype(np.float64))
    with np.errstate(invalid='ignore', divide='ignore'):
        qH = np.nanmax(np.where(bH > 0, eH / bH, 0.0)) if m.any() else 0.0
        qB = np.nanmax(np.where(bB > 0, eB / bB, 0.0)) if m.any() else 0.0
    print('gappy', tag, kind, 'worst error / bar: H', qH, 'B', qB)
    assert np.all(eH <= bH) and np.all(eB <= bB), (tag, kind, qH, qB)


F64 = ('f64', 'f64')
ALL = [F64, ('f64', 'f32'), ('f32', 'f64'), ('f32', 'f32')]
# (r, k, ldu_pad, ldx_pad, mask stride = 1 | k): every tile count of the basis (1, 2, 4, 8 tiles, partial tiles at 3 and 37),
# k = 1, a partial X tile, a full slice, a ragged second slice (70 = 64 + 6) whose launch forms no H
SHAPES = [(3, 1, 0, 0, 1), (3, 5, 2, 3, 'k'), (16, 64, 0, 0, 'k'), (16, 70, 2, 0, 1), (37, 70, 6, 3, 1), (37, 1, 0, 0, 1),
          (64, 5, 0, 0, 'k'), (64, 70, 2, 0, 1), (128, 1, 6, 0, 1), (128, 64, 0, 3, 'k'), (128, 70, 0, 0, 1), (128, 5, 2, 3, 'k')]
EVERY_STORAGE = {(3, 5), (37, 70), (128, 64)}
CASES = [(s, st) for s in SHAPES for st in (ALL if s[:2] in EVERY_STORAGE else [F64])]


@pytest.mark.parametrize('shape,store', CASES, ids=[f'r{s[0]}-k{s[1]}-m{s[4]}-u{st[0]}-x{st[1]}' for s, st in CASES])
def test_kernel_against_numpy(eng, shape, store):
    r, k, ldu_pad, ldx_pad, ldm = shape
    c = _case(eng, r, k, store, seed=900 + r + k, ldu_pad=ldu_pad, ldx_pad=ldx_pad)
    c['mu_d'], c['scale_d'] = eng.to_device(c['mu']), eng.to_device(c['scale'])
    width = 1 if ldm == 1 else max(k, 3)
    # the longdouble products of the fully observed block at r = 128 take seconds: there 'ones' runs for k = 1 only
    kinds = [m for m in MASKS if not (m == 'ones' and r == 128 and k > 1)]
    for kind in kinds:
        _check(eng, c, kind, width, (shape, store))


def _chunked_reference(c, m):
    """long block: f64 BLAS over 512 observed rows (within 512 eps of the chunk's sum of |terms|), longdouble across chunks"""
    obs = np.flatnonzero(m)
    feat = np.minimum((c['row0'] + obs) // c['n_points'], c['F'] - 1)
    x0 = (c['X'][obs] - c['mu'][obs][:, None]) / c['scale'][feat][:, None]
    U = c['U'][obs]
    H, B = np.zeros((c['r'], c['r']), dtype=LD), np.zeros((c['k'], c['r']), dtype=LD)
    for i0 in range(0, len(obs), 512):
        H += U[i0:i0 + 512].T @ U[i0:i0 + 512]
        B += x0[i0:i0 + 512].T @ U[i0:i0 + 512]
    ref = dict(H=H, B=B, SH=np.abs(U).T @ np.abs(U), SB=np.abs(x0).T @ np.abs(U))
    return (ref,) + bars_of(ref, c['n'], c['r'], tighten=512)


def test_kernel_many_panels(eng):
    """features of 100 003 cells, a block of 238 909 rows, 10 % of them observed: every workgroup runs its steady-state
    panel loop, with panels that are skipped and panels whose MFMA steps are"""
    r, k = 64, 17
    c = _case(eng, r, k, F64, seed=1700, long=True)
    c['mu_d'], c['scale_d'] = eng.to_device(c['mu']), eng.to_device(c['scale'])
    m = np.random.default_rng(5).random(c['n']) < 0.1
    m[40_000:60_000] = False                                      # a run of empty panels longer than one scan
    md = _device_mask(eng, m, 1)
    out = _run(eng, c, c['Xd'], md)
    assert np.array_equal(out, _run(eng, c, c['Xd'], md))
    H, B = out[:r * r].reshape(r, r), out[r * r:r * r + k * r].reshape(k, r)
    assert np.array_equal(H, H.T) and out[-1] == m.sum()
    ref, bH, bB = _chunked_reference(c, m)
    eH = np.abs((H.astype(LD) - ref['H']).astype(np.float64))
    eB = np.abs((B.astype(LD) - ref['B']).astype(np.float64))
    print('gappy long block: worst error / bar: H', (eH / bH).max(), 'B', (eB / bB).max())
    assert np.all(eH <= bH) and np.all(eB <= bB)


def test_range_and_refusals(eng):
    import torch
    from openmeasure_amd import _lib
    c = _case(eng, 129, 2, F64, seed=3)
    mu, sc = eng.to_device(c['mu']), eng.to_device(c['scale'])
    md = _device_mask(eng, np.ones(c['n'], dtype=bool), 1)
    with pytest.raises(ValueError, match='128'):
        eng.gappy_normal(c['Ud'], c['row0'], c['n_points'], c['F'], mu, sc, c['Xd'], md)
    # the C entry point itself: SPR_E_INVALID with a message, nothing launched (the outputs keep their bytes)
    lib = _lib.load()
    assert lib.spr_gappy_normal_workspace(129, 2, c['F']) == 0
    out = torch.full((129 * 129 + 2 * 129 + 1,), 7.0, dtype=torch.float64, device='cuda:0')
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda:0')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.spr_gappy_normal_f64(p(c['Ud']), c['n'], 129, c['Ud'].stride(0), p(c['Xd']), 2, c['Xd'].stride(0), c['row0'],
                                  c['n_points'], c['F'], p(mu), p(sc), p(md), 1, p(out), p(out[129 * 129:]), p(out[-1:]),
                                  p(ws), ws.numel(), None)
    assert rc == -1 and b'129' in lib.spr_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    c = _case(eng, 6, 3, F64, seed=1)
    mu, sc = eng.to_device(c['mu']), eng.to_device(c['scale'])
    md = _device_mask(eng, np.ones(c['n'], dtype=bool), 1)
    with pytest.raises(ValueError):
        eng.gappy_normal(c['Ud'], c['row0'], c['n_points'], c['F'], mu, sc, c['Xd'][:-1], md[:-1])
    with pytest.raises(ValueError):
        eng.gappy_normal(c['Ud'], c['row0'], c['n_points'], c['F'], mu, sc, c['Xd'], md[:-1])
    with pytest.raises(TypeError):
        eng.gappy_normal(c['Ud'], c['row0'], c['n_points'], c['F'], mu, sc, c['Xd'], md.to(torch.float64))
    with pytest.raises(ValueError):                               # a stride that walks out of the mask tensor
        eng.gappy_normal(c['Ud'], c['row0'], c['n_points'], c['F'], mu, sc, c['Xd'], md, ldm=2)


@pytest.mark.parametrize('basis', ['f64', 'f32'])
def test_public_method_end_to_end(eng, basis):
    """fit on a small synth case, then gappy_transform against lstsq on the object's own host arrays, at the host test's bar"""
    from openmeasure_amd.rom import DeviceMatrix
    from openmeasure_amd.sparse_sensing import ROM
    from openmeasure_amd.synth import make_R
    n_points, F, m, r = 1531, 3, 24, 8
    t = eng.torch
    dt = t.float32 if basis == 'f32' else t.float64
    R = eng.to_device(make_R(m, r, seed=7))
    Xd = eng.synth(n_points * F, m, 0, n_points, R, 1e-3, 7, dtype=dt)
    Xt_d = eng.synth(n_points * F, m, 0, n_points, R, 1e-3, 8, dtype=dt)[:, :6]     # held out: another seed; ldx = m
    rom = ROM(DeviceMatrix(Xd, basis=basis), F, None, engine=eng)
    rom.fit(select_modes='number', n_modes=r)
    Xt = eng.to_host(Xt_d.contiguous()).astype(np.float64)
    n = Xt.shape[0]
    rng = np.random.default_rng(3)
    three = rng.random((n, 3)) < 0.5
    three[:, 2] = False
    three[n_points:2 * n_points, 2] = True                          # one feature of three observed everywhere
    order = [0, 1, 0, 2, 1, 2]
    M = three[:, order]
    A, cov = rom.gappy_transform(Xt_d, M, return_cov=True)
    info = rom.gappy_info_
    assert info['groups'] == 3 and info['passes'] == 3 and info['group'].tolist() == order
    check_against_lstsq(rom, Xt, M, A)
    np.testing.assert_array_equal(rom.gappy_transform(Xt_d, eng.to_device(M.astype(np.uint8), dtype=t.uint8)), A)
    # mask=None: observed where finite
    Xh = Xt_d.contiguous().clone()
    Xh[eng.to_device((~M).astype(np.uint8), dtype=t.uint8).bool()] = float('nan')
    np.testing.assert_array_equal(rom.gappy_transform(Xh), A)
    assert rom.gappy_info_['groups'] == 3
    std = rom.reconstruct_std(cov=1e-4 * cov)
    assert std.shape == (n, 6) and np.all(np.isfinite(std))
    e = rom.reconstruction_error(Xt_d, Ar=A)
    e0 = rom.reconstruction_error(Xt_d)
    print('end to end', basis, 'repair rel_l2_total', e['rel_l2_total'], 'truncation error of the basis', e0['rel_l2_total'])


# A caller with no Python and no torch in the process: spr_gappy_normal_f64 on hipMalloc'ed memory against loops on the host,
# at the bars of the module docstring (the sums formed here in long double).
C_GAPPY_SRC = r'''
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <hip/hip_runtime_api.h>
#include "spr_hip.h"
#define CK(x) do { if ((x) != 0) { printf("fail %s line %d: %s\n", #x, __LINE__, spr_last_error()); return 1; } } while (0)
int main(void) {
  const int64_t n_points = 2048, row0 = 1000, n = 4999; const int F = 3, r = 6, k = 3, ldu = 8, ldx = 5, ldm = 2;
  double *U = (double *)malloc(sizeof(double) * n * ldu), *X = (double *)malloc(sizeof(double) * n * ldx);
  double *mu = (double *)malloc(sizeof(double) * n), sc[3] = {2.0, 0.5, 1.25}, out[36 + 18 + 1];
  uint8_t *M = (uint8_t *)malloc(n * ldm);
  uint64_t s = 4242;
  for (int64_t i = 0; i < n * ldu; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; U[i] = (double)(s >> 11) / 9007199254740992.0 - 0.5; }
  for (int64_t i = 0; i < n * ldx; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; X[i] = (double)(s >> 11) / 9007199254740992.0 * 3.0; }
  for (int64_t i = 0; i < n; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; mu[i] = (double)(s >> 11) / 9007199254740992.0 + 1.0; }
  for (int64_t i = 0; i < n; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; M[i * ldm] = (s >> 40) % 3 == 0; M[i * ldm + 1] = 1; }
  for (int64_t i = 0; i < n; ++i) if (!M[i * ldm]) for (int j = 0; j < k; ++j) X[i * ldx + j] = NAN;   /* never used */
  if (spr_gappy_normal_f64(NULL, n, r, ldu, NULL, k, ldx, row0, n_points, F, NULL, NULL, NULL, ldm, NULL, NULL, NULL, NULL, 0, NULL) != SPR_E_INVALID) return 2;
  double *dU, *dX, *dmu, *dsc, *dout; uint8_t *dM; void *ws;
  size_t wsb = spr_gappy_normal_workspace(r, k, F);
  if (wsb == 0) return 3;
  CK(hipMalloc((void **)&dU, sizeof(double) * n * ldu)); CK(hipMalloc((void **)&dX, sizeof(double) * n * ldx));
  CK(hipMalloc((void **)&dmu, sizeof(double) * n)); CK(hipMalloc((void **)&dsc, sizeof(sc))); CK(hipMalloc((void **)&dout, sizeof(out)));
  CK(hipMalloc((void **)&dM, n * ldm)); CK(hipMalloc(&ws, wsb));
  CK(hipMemcpy(dU, U, sizeof(double) * n * ldu, hipMemcpyHostToDevice)); CK(hipMemcpy(dX, X, sizeof(double) * n * ldx, hipMemcpyHostToDevice));
  CK(hipMemcpy(dmu, mu, sizeof(double) * n, hipMemcpyHostToDevice)); CK(hipMemcpy(dsc, sc, sizeof(sc), hipMemcpyHostToDevice));
  CK(hipMemcpy(dM, M, n * ldm, hipMemcpyHostToDevice));
  CK(spr_gappy_normal_f64(dU, n, r, ldu, dX, k, ldx, row0, n_points, F, dmu, dsc, dM, ldm, dout, dout + 36, dout + 54, ws, wsb, NULL));
  CK(hipMemcpy(out, dout, sizeof(out), hipMemcpyDeviceToHost));
  double worst = 0.0, cnt = 0.0;
  for (int64_t i = 0; i < n; ++i) cnt += M[i * ldm] != 0;
  if (out[54] != cnt) { printf("nobs %g, expected %g\n", out[54], cnt); return 5; }
  for (int a = 0; a < r + k; ++a)
    for (int c = 0; c < r; ++c) {
      long double ref = 0.0L, sum = 0.0L;
      for (int64_t i = 0; i < n; ++i) {
        if (!M[i * ldm]) continue;
        const double left = a < r ? U[i * ldu + a] : (X[i * ldx + a - r] - mu[i]) / sc[(row0 + i) / n_points];
        ref += (long double)left * U[i * ldu + c]; sum += fabsl((long double)left * U[i * ldu + c]);
      }
      const double got = a < r ? out[a * r + c] : out[36 + (a - r) * r + c];
      const double q = (double)(fabsl((long double)got - ref) / ((n + r + 4) * 0x1p-53L * sum));
      if (!(q <= worst)) worst = q;
      if (a < r && out[a * r + c] != out[c * r + a]) { printf("H is not symmetric\n"); return 6; }
    }
  if (!(worst <= 1.0)) { printf("gappy mismatch: error / bar = %g\n", worst); return 4; }
  printf("C gappy ok: worst error / bar %.3g\n", worst);
  return 0;
}
'''


def test_plain_c_caller_of_gappy_normal(tmp_path):
    if shutil.which('gcc') is None or not os.path.exists('/opt/rocm/include/hip/hip_runtime_api.h'):
        pytest.skip('gcc / HIP runtime headers not available')
    lib = os.path.join(ROOT, 'openmeasure_amd', 'libspr_hip.so')
    src = tmp_path / 'g.c'
    src.write_text(C_GAPPY_SRC)
    exe = tmp_path / 'g'
    subprocess.run(['gcc', '-std=gnu99', '-D__HIP_PLATFORM_AMD__', '-I', os.path.join(ROOT, 'include'),
                    '-I', '/opt/rocm/include', str(src), '-o', str(exe), lib, '-L/opt/rocm/lib', '-lamdhip64', '-lm',
                    '-Wl,-rpath,' + os.path.dirname(lib), '-Wl,-rpath,/opt/rocm/lib'], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert 'C gappy ok' in out.stdout

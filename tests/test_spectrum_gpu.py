"""The eigen half of spectrum_kernel (csrc/spectrum.hip: Jacobi sweeps, sort, sign rule, floor on S, W, Ar, expvar, info) on
the GPU, on the hard spectra of tests/test_spectrum_host.py at every m from 1 to 64.  That file holds the NumPy transcription
of the kernel, the catalogue, the checker and, in its docstring, THE BARS with where they come from; the transcription passes
the same checks there, and seven mutations of it do not.

The Gram matrix goes straight to eng.spectrum with F = 1, scale_type = 'none' and fstats = [[[1, 0, 0]]]: the scale is exactly
1 (asserted) and the kernel's A is G bit for bit.  Every case goes through check(); none is left out because it ended at the
sweep limit (the capped bar applies there); for m <= 24 fit()'s verdict (info[0] < 15 or info[1] <= 1e-24 info[2]) is
asserted as well.  Every case prints its sweeps, off^2 / diag^2 and each error over its bar.

Largest error / bar over the catalogue at the fourteen m and Wishart / two clusters at every m (BAR_ORTH = 8 comes from the
transcription alone: twice its worst, 3.6 m u):
  check           transcription   MI355X
  orthogonality   0.45            0.18   (1.4 m u)
  residual        0.75            0.33
  eigenvalues     0.70            0.38
  offdiag         0.29            0.28
  info[2]         0.13            0.15
  S               0.50 ulp        0.50 ulp
  W               0.50 of 2 ulp   0.50 of 2 ulp
  Ar              0.50 ulp        0.50 ulp
  expvar          0.08            0.08
Sweeps on the MI355X: DESIGN.md has the table per family at m = 24 and 64.  For m <= 24 every catalogue input meets the
verdict (two clusters at m = 24 needs 14 sweeps, the most); from m = 25 up 66 (m, input) pairs run to the limit: Wishart,
indefinite and rank deficient stalled at off^2 / diag^2 = 1-3e-31, two clusters and the graded spectra still converging (up to
2.9e-17, two clusters at m = 58).  The end-to-end fits stay on the all-device route (_device_fit_fallback_ False); Sigma_r error
/ bar 0.010 there and 0.002 on the host route, reconstruction 5e-15 and 4e-15 relative."""
import numpy as np
import pytest

from tests.test_spectrum_host import KEYS, MS, U, accept, case, cases, fmt, merge, norm2, rs_of

pytestmark = pytest.mark.gpu
LD = np.longdouble
WORST = {}                                                  # largest error / bar over the tests that ran so far (printed)


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def run(eng, G, r):
    """eng.spectrum on A = G: one feature, scale 1"""
    sp = eng.spectrum(eng.to_device(np.array(G, dtype=np.float64)[None]), eng.to_device(np.array([[[1.0, 0.0, 0.0]]])), 'none', r)
    out = {k: eng.to_host(sp[k]) for k in KEYS}
    assert eng.to_host(sp['scale'])[0] == 1.0 and eng.to_host(sp['inv_scale'])[0] == 1.0
    return out


def report(tag, out, res):
    with np.errstate(all='ignore'):
        print(f'{tag}: sweeps {int(out["info"][0])} off2/diag2 {out["info"][1] / out["info"][2]:.1e} error / bar {fmt(res)}')


@pytest.mark.parametrize('m', MS)
def test_catalogue(eng, m):
    """the whole catalogue, r in {1, m} (and m // 2 at m = 24 and 64)"""
    for c in cases(m):
        for r in rs_of(m):
            out = run(eng, c.G, r)
            res = accept(c.G, out, r, c.exact)
            merge(WORST, res)
            report(f'm={m} r={r} {c.name}', out, res)
    print('worst so far: ' + fmt(WORST))


@pytest.mark.parametrize('m0', [1, 17, 33, 49])
def test_every_m(eng, m0):
    """Wishart and two clusters at every m from 1 to 64"""
    for m in range(m0, m0 + 16):
        for name in ('wishart', 'two clusters'):
            c = case(m, name)
            out = run(eng, c.G, m)
            res = accept(c.G, out, m)
            merge(WORST, res)
            report(f'm={m} {name}', out, res)
    print('worst so far: ' + fmt(WORST))


@pytest.mark.parametrize('m', [7, 24, 41, 64])
def test_two_calls_are_bit_identical(eng, m):
    """fixed pairing, fixed reduction order: every rank of a sharded run computes the same factors"""
    for name in ('wishart', 'two clusters', 'graded 1e-16', 'underflow trigger'):
        G = case(m, name).G
        a, b = run(eng, G, m // 2), run(eng, G, m // 2)
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (m, name, k)


@pytest.mark.parametrize('m', [4, 5, 24])
def test_underflow_trigger(eng, m):
    """two exactly equal diagonal entries with 1e-200 between them: w == 0 and u^2 underflows in the first rotation"""
    G = case(m, 'underflow trigger').G
    out = run(eng, G, m)
    for k in KEYS:
        assert np.all(np.isfinite(out[k])), k
    assert np.sum(np.abs(out['lam'] - 1.0) <= 4 * m * U * norm2(G)) == 2
    res = accept(G, out, m)
    report(f'm={m} underflow trigger', out, res)


def test_nan_entry_shows_in_the_first_singular_value(eng):
    """what _device_fit looks at before it trusts the factors; the call returns (the sort is total: order[] is a permutation)"""
    G = np.array(case(5, 'wishart').G)
    G[1, 3] = G[3, 1] = np.nan
    out = run(eng, G, 2)
    assert not np.isfinite(out['S'][0])


# ------------------------------------------------------------------------------------------------ end to end
def clustered(s, seed):
    """X = U diag(s) W^T, (400, 24): the columns of W orthonormal and orthogonal to the ones vector, so that row centring
    leaves the singular values s"""
    rng = np.random.default_rng(seed)
    n, m, k = 400, 24, len(s)
    Uo = np.linalg.qr(rng.standard_normal((n, k)))[0]
    Wo = np.linalg.qr(np.column_stack([np.ones(m), rng.standard_normal((m, k))]))[0][:, 1:]
    assert np.max(np.abs(Wo.T @ np.ones(m))) < 1e-14
    return (Uo * np.asarray(s)) @ Wo.T


@pytest.mark.parametrize('route', ['default', 'host'])
@pytest.mark.parametrize('name,s,r', [('clusters 8 + 15', [2.0] * 8 + [1.0] * 15, 8), ('one + 22 equal', [3.0] + [1.0] * 22, 1)],
                         ids=['clusters', 'one-apart'])
def test_fit_on_degenerate_spectra(eng, monkeypatch, name, s, r, route):
    """ROM.fit at m = 24 on data whose Gram matrix has whole clusters of equal eigenvalues, r on the cluster boundary, on the
    all-device route and on the host route, against the LAPACK SVD of the centred matrix"""
    import openmeasure_amd.rom as rom_mod
    from openmeasure_amd.rom import ROM
    n_points, F, m = 200, 2, 24
    n = F * n_points
    X = clustered(s, 77)
    Xl = X.astype(LD)
    cnt = Xl.sum(axis=1) / m
    X0 = np.asarray(Xl - cnt[:, None], dtype=np.float64)
    Uu, S, Vt = np.linalg.svd(X0, full_matrices=False)
    if route == 'host':
        monkeypatch.setattr(rom_mod, '_DEVICE_SPECTRUM_MAX_M', 0)
    rom = ROM(X, F, None, engine=eng)
    rom.fit(scale_type='none', axis_cnt=1, select_modes='number', n_modes=r)
    print(f'{name} {route}: _device_fit_fallback_ = {getattr(rom, "_device_fit_fallback_", False)}')
    fro2 = float(np.sum(S * S))
    bar_S = ((n + 2) * U * fro2 + 4 * m * U * S[0] ** 2) / (2 * S[:r]) + m * U * S[0]
    err_S = np.abs(rom.Sigma_r - S[:r])
    print(f'{name} {route}: Sigma_r error / bar {np.max(err_S / bar_S):.3f}')
    assert rom.Sigma_r.shape == (r,) and np.all(err_S <= bar_S), (err_S, bar_S)
    np.testing.assert_allclose(rom.exp_variance_, (100 * np.cumsum(S * S) / np.sum(S * S))[:r], rtol=1e-10)
    want = (Uu[:, :r] * S[:r]) @ Vt[:r, :3] + np.asarray(cnt, dtype=np.float64)[:, None]
    got = rom.reconstruct(rom.Ar[:3])
    assert got.shape == (n, 3)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f'{name} {route}: reconstruct rel_fro {rel:.2e}')
    assert rel <= 1e-9, rel

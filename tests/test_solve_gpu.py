"""The predict kernels of csrc/solve.hip and csrc/solve_pinv.hip (eng.solve_ols, eng.solve_pinv) on every rung of the padded
width, on both sides of each boundary, against np.linalg.pinv(W Theta) in float64 as the oracle's predict_ols computes it.

Shapes.  solve_ols_kernel<NT> is picked by need = ceil((r + 2) / 16): r = 1, 14 (NT 1); 15, 30 (NT 2); 31, 46 (NT 3); 47, 78
(NT 5); 79, 128 (NT 9).  For each r: s = r, r + 1, r + 15, r + 17, r + 33, 2 r + 5 -- a single ragged panel, several panels,
a last panel of one sensor -- and, once per rung, an s that is an exact multiple of the panel height (32 sensors; 16 for
NT 9).  r = 129, the first width of the workspace kernels, with s = 129 and 146 through solve_ols and solve_pinv.

Inputs.  Theta = U diag(logspace(0, -log10(cond), r)) V^T with random orthogonal factors, cond = 1 and 1e2; three features
with their own scale, a random centre per sensor; three vectors in one call: unweighted, weighted, weighted.

Bars, per vector, kappa = cond_2(W Theta):
    |a - a_ref|_2 <= 50 kappa 2.2e-16 |a_ref|_2,   the same for sigma_a against |pinv(W Theta) y0_sigma|
(the factor 50 is that of tests/test_gpu_parity.test_predict_ill_conditioned_goes_through_svd).  The kernel's algorithm --
equilibrated normal equations, Cholesky, one refinement step -- written in NumPy reaches at most 0.24 of this bar over
these shapes.  Exact: y0 (one subtraction, one division), Ar_sigma of the unweighted vector is zero, info[:, 0] == 0.
info[:, 1], the pivots' ratio (max L_jj / min L_jj)^2, is not held to cond(W Theta D)^2: it is a lower estimate, and on
these inputs it lies between 0.0092 and 1.0 of it.

Worst error / bar seen on an MI355X: solve_ols at r <= 128 0.250, solve_ols at r = 129 0.147, solve_pinv at r = 129 0.298
-- the same on the build before this file and on the builds whose kernels were moved onto shared helpers (LAB_NOTEBOOK, "One
dense-solve core"): their outputs agree bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = 2.2e-16
SCALE = np.array([1.0, 25.0, 0.04])                          # three features with different scl
RS = [1, 14, 15, 30, 31, 46, 47, 78, 79, 128]
PANEL_MULTIPLE = {14: 32, 30: 64, 46: 64, 78: 96, 128: 144}  # one s per rung that fills its last panel


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def sensor_counts(r):
    return [r, r + 1, r + 15, r + 17, r + 33, 2 * r + 5] + ([PANEL_MULTIPLE[r]] if r in PANEL_MULTIPLE else [])


def draw(s, r, cond, seed):
    """Theta (s, r) with singular values logspace(0, -log10(cond), r), cnt (s,), y (3, s, 3): unweighted, weighted, weighted"""
    rng = np.random.default_rng(seed)
    Uq, _ = np.linalg.qr(rng.standard_normal((s, r)))
    Vq, _ = np.linalg.qr(rng.standard_normal((r, r)))
    Theta = (Uq * np.logspace(0, -np.log10(cond), r)) @ Vq.T
    cnt = rng.standard_normal(s)
    y = np.zeros((3, s, 3))
    for p in range(3):
        fid = rng.integers(0, 3, s)
        v0 = Theta @ rng.standard_normal(r) + 1e-3 * rng.standard_normal(s)
        y[p, :, 0] = v0 * SCALE[fid] + cnt
        if p > 0:
            y[p, :, 1] = 0.05 * (1.0 + rng.random(s)) * SCALE[fid]
        y[p, :, 2] = fid
    return Theta, cnt, y


def reference(Theta, cnt, y):
    """y0 (3, s, 2), a_ref, sigma_ref (3, r), kappa (3,): predict_ols of the oracle, vector by vector"""
    y0 = np.empty(y.shape[:2] + (2,))
    a, sg, kappa = [], [], []
    for p in range(len(y)):
        scl = SCALE[y[p, :, 2].astype(int)]
        y0[p, :, 0] = (y[p, :, 0] - cnt) / scl
        y0[p, :, 1] = y[p, :, 1] / scl
        weighted = bool(np.any(y[p, :, 1]))
        W = np.diag(1 / y0[p, :, 1]) if weighted else np.eye(len(cnt))
        pinv = np.linalg.pinv(W @ Theta)
        a.append(pinv @ (W @ y0[p, :, 0]))
        sg.append(np.abs(pinv @ y0[p, :, 1]) if weighted else np.zeros(Theta.shape[1]))
        kappa.append(np.linalg.cond(W @ Theta))
    return y0, np.array(a), np.array(sg), np.array(kappa)


def check(eng, solve, Theta, cnt, y, tag):
    """one engine call against the reference -> the worst error / bar of its three vectors"""
    Ar, As, y0, info = (eng.to_host(t) for t in solve(eng.to_device(Theta), eng.to_device(cnt), eng.to_device(SCALE),
                                                       eng.to_device(y)))
    y0_ref, a_ref, s_ref, kappa = reference(Theta, cnt, y)
    assert np.array_equal(y0, y0_ref), tag
    assert not As[0].any(), tag
    worst = 0.0
    for p in range(3):
        bar = 50 * kappa[p] * EPS
        worst = max(worst, np.linalg.norm(Ar[p] - a_ref[p]) / (bar * np.linalg.norm(a_ref[p])))
        if p > 0:
            worst = max(worst, np.linalg.norm(As[p] - s_ref[p]) / (bar * np.linalg.norm(s_ref[p])))
    print(f'{solve.__name__} {tag}: worst error / bar {worst:.3f}')
    assert worst <= 1.0, (tag, worst)
    return info, worst


@pytest.mark.parametrize('cond', [1.0, 1e2])
@pytest.mark.parametrize('r', RS)
def test_solve_ols_every_rung_both_sides(eng, r, cond):
    worst = 0.0
    for s in sensor_counts(r):
        Theta, cnt, y = draw(s, r, cond, seed=1000 * r + s + int(cond))
        info, w = check(eng, eng.solve_ols, Theta, cnt, y, (s, r, cond))
        assert info.shape == (3, 2) and np.all(info[:, 0] == 0), (s, r, cond, info)
        worst = max(worst, w)
    print(f'solve_ols r={r} cond={cond:g}: worst error / bar over its sensor counts {worst:.3f}')


@pytest.mark.parametrize('cond', [1.0, 1e2])
@pytest.mark.parametrize('s', [129, 146])
def test_first_wide_width(eng, s, cond):
    r = 129
    Theta, cnt, y = draw(s, r, cond, seed=1000 * r + s + int(cond))
    info, _ = check(eng, eng.solve_ols, Theta, cnt, y, (s, r, cond))
    assert info.shape == (3, 2) and np.all(info[:, 0] == 0), info
    info, _ = check(eng, eng.solve_pinv, Theta, cnt, y, (s, r, cond))
    assert np.all(info[:, 0] > 0) and np.all(info[:, 1] == r), info          # Jacobi converged, full rank kept

"""The eigen half of spectrum_kernel (csrc/spectrum.hip, steps 3 and 4: Jacobi sweeps, sort, sign rule, floor on S, W, Ar,
expvar, info) on hard spectra at every m.  This file holds what tests/test_spectrum_gpu.py shares with it -- a NumPy
transcription of the kernel, the input catalogue, the checker -- and proves here, on the CPU, that the three work: the
transcription passes the checker on the whole catalogue, and seven deliberate mutations of it do not.

THE TRANSCRIPTION (spectrum) follows the kernel line by line in plain float64: the same round-robin pairing pair_of, the
same rotation formula with its reciprocal / reciprocal-square-root Newton steps, rows then columns of A then columns of V,
the same stop test off^2 <= 1e-31 diag^2 measured BEFORE a sweep, the counting sort with its index tie-break, the sign of the
first largest entry, floor = S_0 sqrt(m 2.22e-16) (1 when that is not positive), W = V / max(S, floor), Ar = V S, expvar = 100
cumsum(max(lam, 0)) / sum, info = (sweeps, off^2, diag^2).  It has no fma and sums in another order, so its sweep counts and
its last bits are its own: it is the proof that the bars can be met, not a prediction of the device's figures.
rotation(..., fixed=False) is the formula before the underflow fix: h2 = w^2 + u^2 is exactly zero when w == 0 and |u| <
~2e-162, fast_rsqrt(0) is inf * (-0 * inf ...) = NaN, and every output becomes NaN.  The fixed formula takes t from w / sc,
u / sc (sc = max(|w|, |u|)) whenever h2 is not a positive normal number -- zero, among the denormals, where it has lost its digits, or
overflowed -- and the old instructions otherwise.

THE CATALOGUE cases(m, seed): identity; diagonal 1..m permuted; diagonal with repeats; 1 1^T; 1 1^T + I; two clusters; a tight
cluster; graded 1e-12 and 1e-16; rank deficient; Wishart; Toeplitz; Wilkinson; indefinite; for m a power of two a Hadamard
similarity of small integers (entries and eigen-system exact); for m >= 4 the underflow trigger blockdiag([[1, 1e-200],
[1e-200, 1]], [[2, 1], [1, 3]], 4, 5, ...).

THE BARS (u = 2.22e-16, capped: info[0] == 15; all algebra in np.longdouble on G as uploaded).
* residual |G V - V diag(lam)|_2 and eigenvalues max |lam - eigvalsh(G)| (the exact integers for the Hadamard case):
  4 m u |G|_2, the project's constant for a symmetric eigen-solver (tests/test_scaling_host.py), + sqrt(info[1]) when capped.
* info is honest on one side: |offdiag(V^T G V)|_F <= sqrt(info[1]) + 4 m u |G|_F; info[2] within 8 m u of |diag(V^T G V)|_F^2.
* orthogonality max |V^T V - I| <= BAR_ORTH m u.  The project has no constant for it; BAR_ORTH = 8 is twice the worst of the
  transcription over the catalogue and the every-m sweep (3.6 m u, rank deficient at m = 23:
  test_orthogonality_bar_is_twice_the_transcriptions_worst measures it on every run), rounded up to an integer.
* S = sqrt(max(lam, 0)) to 1 ulp, Ar = V S to 1 ulp, W = V / max(S, floor) to 2 ulp (floor evaluated in float64 exactly as the
  kernel does: one product of S_0 with the correctly rounded sqrt(m 2.22e-16)), expvar to 8 m u relative.
* exact: lam non-increasing, expvar non-decreasing, the sign rule, the shapes, and for diagonal input zero sweeps, V the
  permutation matrix of the stable descending sort, lam bit-equal to the sorted diagonal.
  The Wilkinson matrix enters at m >= 2: at m = 1 it is the zero matrix, whose expvar is 0 / 0 in the reference as well.
Largest error / bar of the transcription over everything this file runs (where): residual 0.75 and eigenvalues 0.70 (two
clusters, m = 20), orthogonality 0.45 (rank deficient, m = 23), offdiag 0.29 (two clusters, m = 62), info[2] 0.13, S 0.50 ulp,
W 0.50 of 2 ulp, Ar 0.50 ulp, expvar 0.08 (the device's are in the GPU file's docstring).

fit()'s verdict (verdict): info[0] < 15 or info[1] <= 1e-24 info[2].  The transcription meets it on the whole catalogue for
m <= 24 (asserted here), although rank deficient, indefinite and graded inputs already run to the limit at m = 23 and 24: they
stall at off^2 / diag^2 = 1.1e-31, the rounding floor, a hair above the 1e-31 of the stop test.  From m = 25 upwards two clusters
and the graded inputs end at the limit still converging, with off^2 / diag^2 up to 1e-17, and pass through the capped bar.  The one mutation that keeps every output honest -- a rotation skipped in
each round, so that the last row is never annihilated -- is caught by the verdict alone, which is why accept() is check() plus
the verdict at m <= 24, in both files."""
import collections
import functools

import numpy as np
import pytest

LD = np.longdouble
U = 2.220446049250313e-16                                  # the kernel's own constant in its floor
TINY = float(np.finfo(np.float64).tiny)                     # the smallest positive normal double
MAX_SWEEPS = 15                                         # SP_MAX_SWEEPS
BAR_ORTH = 8                                                # in units of m u: see the module docstring
MS = (1, 2, 3, 4, 7, 8, 16, 23, 24, 25, 32, 41, 63, 64)
KEYS = ('lam', 'S', 'expvar', 'V', 'W', 'Ar', 'info')
f64 = lambda a: np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the transcription
def pair_of(k, rd, mp):
    """pair k of round rd in the round-robin tournament over mp (even) indices, p < q"""
    if k == 0:
        a, b = mp - 1, rd % (mp - 1)
    else:
        a, b = (rd + k) % (mp - 1), (rd - k + (mp - 1)) % (mp - 1)
    return (a, b) if a < b else (b, a)


@functools.lru_cache(maxsize=None)
def pairing(mp):
    """(mp - 1, mp / 2) index arrays p, q of every round"""
    pq = np.array([[pair_of(k, rd, mp) for k in range(mp // 2)] for rd in range(mp - 1)])
    return pq[:, :, 0], pq[:, :, 1]


def fast_rcp(x):
    y = 1.0 / x
    y = (-x * y + 1.0) * y + y
    y = (-x * y + 1.0) * y + y
    return y


def fast_rsqrt(x):
    y = 1.0 / np.sqrt(x)
    h = 0.5 * x
    y = y * (-h * y * y + 1.5)
    y = y * (-h * y * y + 1.5)
    return y


def rotation(app, aqq, apq, fixed=True):
    """(c, s) of the rotations that annihilate a_pq, for arrays of pairs"""
    with np.errstate(all='ignore'):
        u, w = 2.0 * apq, aqq - app
        h2 = w * w + u * u
        t = np.abs(u) * fast_rcp(np.abs(w) + h2 * fast_rsqrt(h2))
        if fixed:
            bad = ~((h2 >= TINY) & (h2 < np.inf))            # not a positive normal number
            if bad.any():                                   # w^2 + u^2 leaves the range: the same formula on w / sc, u / sc
                sc = np.maximum(np.abs(w), np.abs(u))
                ws, us = w / sc, u / sc
                t = np.where(bad, np.abs(us) / (np.abs(ws) + np.sqrt(ws * ws + us * us)), t)
        t = np.where((w >= 0.0) == (u >= 0.0), t, -t)
        c = fast_rsqrt(t * t + 1.0)
        on = np.abs(apq) > 1e-300
        return np.where(on, c, 1.0), np.where(on, t * c, 0.0)


def nonneg(l):
    """max(l, 0) that keeps a NaN"""
    return l if (l > 0.0 or l != l) else 0.0


def sort_order(lam, total=True, reverse_tie=False):
    """order[rank] = index, descending; total: NaN counts as the largest value, so that order is a permutation for any input"""
    m = len(lam)
    order = np.full(m, -1)
    for i in range(m):
        li, rank = lam[i], 0
        for j in range(m):
            lj = lam[j]
            if total:
                gt = lj > li or (lj != lj and li == li)
                tie = not gt and not (li > lj or (li != li and lj == lj))
            else:
                gt, tie = lj > li, lj == li
            rank += bool(gt or (tie and (j > i if reverse_tie else j < i)))
        order[rank] = i
    return order


MUTATIONS = ('v_sign', 'pad', 'tie', 'nofloor', 'ar_div', 'expvar_noclamp', 'skip')


def spectrum(G, r, fixed=True, mutate=None):
    """spectrum_kernel steps 3 and 4 on A = G.  mutate: one of MUTATIONS, a deliberately wrong kernel for the teeth test"""
    G = np.asarray(G, dtype=np.float64)
    m = G.shape[0]
    mp = m + (m & 1)
    A = np.zeros((mp, mp))
    if mutate == 'pad':
        A[:] = 1.0                                          # the pad row and column keep what the buffer held
    A[:m, :m] = G
    V = np.zeros((mp, mp))
    V[np.arange(m), np.arange(m)] = 1.0
    P, Q = pairing(mp)
    offmask = ~np.eye(m, dtype=bool)
    sweeps, off2, diag2 = 0, 0.0, 0.0
    with np.errstate(all='ignore'):
        while sweeps < MAX_SWEEPS:
            sq = A[:m, :m] ** 2
            off2, diag2 = float(np.sum(sq[offmask])), float(np.sum(np.diag(sq)))
            if off2 <= 1e-31 * diag2:
                break
            for rd in range(mp - 1):
                p, q = P[rd], Q[rd]
                c, s = rotation(A[p, p], A[q, q], A[p, q], fixed)
                if mutate == 'skip':
                    c[0], s[0] = 1.0, 0.0
                xp, xq = A[p, :].copy(), A[q, :].copy()     # rows: J^T from the left
                A[p, :] = c[:, None] * xp - s[:, None] * xq
                A[q, :] = s[:, None] * xp + c[:, None] * xq
                yp, yq = A[:, p].copy(), A[:, q].copy()     # columns: J from the right
                A[:, p] = c * yp - s * yq
                A[:, q] = s * yp + c * yq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                sv = -s if mutate == 'v_sign' else s
                V[:, p] = c * vp - sv * vq
                V[:, q] = sv * vp + c * vq
            sweeps += 1
        lam0 = np.diag(A)[:m].copy()
        order = sort_order(lam0, total=fixed, reverse_tie=mutate == 'tie')
        lam = lam0[order]
        Vs = V[:m][:, order]
        sgn = np.ones(m)
        for k in range(m):
            best, val = -1.0, 1.0
            for i in range(m):
                v = Vs[i, k]
                if abs(v) > best:
                    best, val = abs(v), v
            sgn[k] = -1.0 if val < 0.0 else 1.0
        Vs = Vs * sgn
        l0 = lam[0] if lam[0] > 0.0 else 0.0
        floor_s = np.sqrt(l0) * np.sqrt(m * 2.220446049250313e-16)
        if not floor_s > 0.0:
            floor_s = 1.0
        S = np.sqrt(np.array([nonneg(l) for l in lam]))
        clamp = (lambda l: l) if mutate == 'expvar_noclamp' else (lambda l: l if l > 0.0 else 0.0)
        tot = np.float64(0.0)
        for l in lam:
            tot += clamp(l)
        expvar, run = np.empty(m), np.float64(0.0)
        for k, l in enumerate(lam):
            run += clamp(l)
            expvar[k] = 100.0 * run / tot
        den = S[:r] if mutate == 'nofloor' else np.where(S[:r] > floor_s, S[:r], floor_s)
        W = Vs[:, :r] / den
        Ar = Vs[:, :r] / S[:r] if mutate == 'ar_div' else Vs[:, :r] * S[:r]
    return dict(lam=lam, S=S, expvar=expvar, V=Vs, W=W, Ar=Ar, info=np.array([float(sweeps), off2, diag2]))


# ------------------------------------------------------------------------------------------------ the catalogue
Case = collections.namedtuple('Case', 'name G exact')      # exact: the eigenvalues where they are known exactly, or None


def hadamard(m):
    H = np.ones((1, 1))
    while H.shape[0] < m:
        H = np.block([[H, H], [H, -H]])
    return H


def trigger(m):
    """two exactly equal diagonal entries with a tiny entry between them, and a block that keeps the sweep going"""
    G = np.diag(np.arange(m, dtype=np.float64))
    G[:2, :2] = [[1.0, 1e-200], [1e-200, 1.0]]
    G[2:4, 2:4] = [[2.0, 1.0], [1.0, 3.0]]
    return G


@functools.lru_cache(maxsize=None)
def cases(m, seed=0):
    """the catalogue of the module docstring: symmetric float64 matrices.  Shared: never written to."""
    rng = np.random.default_rng(7919 * m + seed)
    Q = np.linalg.qr(rng.standard_normal((m, m)))[0]
    sim = lambda d: (Q * np.asarray(d, dtype=np.float64)) @ Q.T
    one = np.ones((m, m))
    idx = np.arange(m)
    k2 = (m + 1) // 2
    rk = max(1, m // 3)
    X = rng.standard_normal((3 * m, m))
    out = [Case('identity', np.eye(m), None),
           Case('diagonal permuted', np.diag(rng.permutation(m) + 1.0), None),
           Case('diagonal repeats', np.diag(1.0 + idx % 3), None),
           Case('ones', one, None),
           Case('ones + I', one + np.eye(m), None),
           Case('two clusters', sim([2.0] * k2 + [1.0] * (m - k2)), None),
           Case('tight cluster', sim(1.0 + 1e-9 * idx), None),
           Case('graded 1e-12', sim(np.logspace(0, -12, m)), None),
           Case('graded 1e-16', sim(np.logspace(0, -16, m)), None),
           Case('rank deficient', (Q[:, :rk] * np.linspace(3.0, 1.0, rk)) @ Q[:, :rk].T, None),
           Case('wishart', X.T @ X, None),
           Case('toeplitz', 0.99 ** np.abs(idx[:, None] - idx[None, :]), None),
           Case('indefinite', sim(np.linspace(1.0, -0.5, m)), None)]
    if m >= 2:                                              # at m = 1 it is the zero matrix, whose expvar is 0 / 0 by definition
        out.append(Case('wilkinson', np.diag(np.abs(idx - (m - 1) / 2.0)) + np.diag(np.ones(m - 1), 1) + np.diag(np.ones(m - 1), -1), None))
    if m & (m - 1) == 0:
        d = 1.0 + (idx * 3) % 4                            # small integers with repeats: H diag(d) H^T / m is exact
        H = hadamard(m)
        out.append(Case('hadamard', (H * d) @ H.T / m, np.sort(d)[::-1]))
    if m >= 4:
        out.append(Case('underflow trigger', trigger(m), None))
    out = [Case(c.name, (c.G + c.G.T) / 2, c.exact) for c in out]
    for c in out:
        c.G.setflags(write=False)
    return tuple(out)


def case(m, name):
    return next(c for c in cases(m) if c.name == name)


# ------------------------------------------------------------------------------------------------ the checker
def ulps(got, want):
    """largest |got - want| in units of the spacing of float64 at want (want in longdouble)"""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(f64(want))).astype(LD)))


def norm2(M):
    return float(np.linalg.norm(f64(M), 2)) if M.size else 0.0


def verdict(info):
    """what fit() asks of the kernel before it stays on the all-device route"""
    return bool(info[0] < MAX_SWEEPS or info[1] <= 1e-24 * info[2])


def check(G, out, r, exact=None):
    """every property of the module docstring on the host arrays of eng.spectrum (or of the transcription).  Returns
    {check: error / bar}; raises AssertionError with the name of the first check that is missed."""
    G = np.asarray(G, dtype=np.float64)
    m = G.shape[0]
    lam, S, expvar, V, W, Ar, info = (np.asarray(out[k], dtype=np.float64) for k in KEYS)
    assert lam.shape == S.shape == expvar.shape == (m,) and V.shape == (m, m) and info.shape == (3,), 'shapes'
    assert W.shape == (m, r) and Ar.shape == (m, r), ('shapes of W and Ar', W.shape, Ar.shape)
    for k in KEYS:
        assert np.all(np.isfinite(out[k])), ('finite', k)
    assert info[0] == int(info[0]) and 0 <= info[0] <= MAX_SWEEPS, ('sweeps', info[0])
    capped = info[0] == MAX_SWEEPS
    res = {}

    def bar(name, err, limit):
        res[name] = float(err / limit) if limit > 0 else (0.0 if err == 0 else np.inf)
        assert err <= limit, (name, float(err), float(limit), 'sweeps', int(info[0]), 'off2/diag2', info[1] / info[2])

    Gl, Vl, laml = G.astype(LD), V.astype(LD), lam.astype(LD)
    g2 = norm2(G)
    slack = np.sqrt(info[1]) if capped else 0.0
    bar('orthogonality', np.max(np.abs(Vl.T @ Vl - np.eye(m))), BAR_ORTH * m * U)
    bar('residual', norm2(Gl @ Vl - Vl * laml), 4 * m * U * g2 + slack)
    ref = np.asarray(exact, dtype=np.float64) if exact is not None else np.linalg.eigvalsh(G)[::-1]
    bar('eigenvalues', np.max(np.abs(laml - ref)), 4 * m * U * g2 + slack)
    T = Vl.T @ Gl @ Vl
    d2 = np.sum(np.diag(T) ** 2)
    offT = np.sqrt(np.sum((T - np.diag(np.diag(T))) ** 2))
    bar('offdiag', offT, np.sqrt(info[1]) + 4 * m * U * float(np.linalg.norm(G)))
    bar('info[2]', abs(LD(info[2]) - d2), 8 * m * U * d2)
    assert np.all(np.diff(lam) <= 0), 'lam is not non-increasing'
    pos = np.maximum(laml, 0)
    bar('S ulp', ulps(S, np.sqrt(pos)), 1.0)
    bar('expvar', np.max(np.abs(expvar - 100 * np.cumsum(pos) / np.sum(pos)) / (100 * np.cumsum(pos) / np.sum(pos))), 8 * m * U)
    assert np.all(np.diff(expvar) >= 0), 'expvar is not non-decreasing'
    top = V[np.argmax(np.abs(V), axis=0), np.arange(m)]
    assert np.all(top > 0), ('sign rule', top)
    floor = S[0] * np.sqrt(m * 2.220446049250313e-16)      # float64, as the kernel evaluates it
    if not floor > 0:
        floor = 1.0
    bar('W ulp', ulps(W, Vl[:, :r] / np.maximum(S[:r], floor).astype(LD)), 2.0)
    bar('Ar ulp', ulps(Ar, Vl[:, :r] * S[:r].astype(LD)), 1.0)
    if not np.any(G - np.diag(np.diag(G))):                 # diagonal input: nothing to rotate
        d = np.diag(G)
        order = np.argsort(-d, kind='stable')               # equal entries keep their index order
        assert info[0] == 0 and info[1] == 0, ('a diagonal matrix needs no sweep', info)
        assert np.array_equal(lam, d[order]), 'lam is not the sorted diagonal bit for bit'
        assert np.array_equal(V, np.eye(m)[:, order]), 'V is not the permutation matrix of the stable sort'
    return res


def accept(G, out, r, exact=None):
    """check(), and fit()'s verdict where fit() takes the kernel's word for it (m <= 24)"""
    res = check(G, out, r, exact)
    if G.shape[0] <= 24:
        assert verdict(out['info']), ('verdict', list(out['info']))
    return res


@functools.lru_cache(maxsize=None)
def transcribed(m, name, r):
    """the transcription's output for a catalogue input.  Shared: never written to."""
    return spectrum(case(m, name).G, r)


def merge(worst, res):
    for k, v in res.items():
        worst[k] = max(worst.get(k, 0.0), v)


def fmt(res):
    return ' '.join(f'{k} {v:.2f}' for k, v in res.items())


def rs_of(m):
    """the r values of the catalogue test: 1 and m, and m // 2 at m = 24 and 64"""
    return sorted({1, m} | ({m // 2} if m in (24, 64) else set()))


# ------------------------------------------------------------------------------------------------ the tests of this file
WORST = {}                                                  # largest error / bar over the tests that ran so far (printed)


@pytest.mark.parametrize('m', MS)
def test_transcription_on_the_catalogue(m):
    for c in cases(m):
        for r in rs_of(m):
            out = transcribed(m, c.name, r)
            res = accept(c.G, out, r, c.exact)
            merge(WORST, res)
            print(f'm={m} r={r} {c.name}: sweeps {int(out["info"][0])} off2/diag2 {out["info"][1] / out["info"][2]:.1e} '
                  f'error / bar {fmt(res)}')
    print('worst so far: ' + fmt(WORST))


@pytest.mark.parametrize('m0', [1, 17, 33, 49])
def test_transcription_at_every_m(m0):
    for m in range(m0, m0 + 16):
        for name in ('wishart', 'two clusters'):
            c = case(m, name)
            out = transcribed(m, name, m)
            res = accept(c.G, out, m)
            merge(WORST, res)
            print(f'm={m} {name}: sweeps {int(out["info"][0])} off2/diag2 {out["info"][1] / out["info"][2]:.1e} error / bar {fmt(res)}')
    print('worst so far: ' + fmt(WORST))


def test_orthogonality_bar_is_twice_the_transcriptions_worst():
    """BAR_ORTH comes from the transcription, not from the device: twice its worst max |V^T V - I| / (m u) over the catalogue at
    the fourteen m and over Wishart / two clusters at every m, rounded up to an integer (the random factor Q depends on the
    LAPACK at hand, so the assertion leaves room: between two and three times the worst)"""
    worst, at = 0.0, None
    todo = [(m, c) for m in MS for c in cases(m)] + [(m, case(m, n)) for m in range(1, 65) for n in ('wishart', 'two clusters')]
    for m, c in todo:
        V = transcribed(m, c.name, m)['V'].astype(LD)
        e = float(np.max(np.abs(V.T @ V - np.eye(m)))) / (m * U)
        if e > worst:
            worst, at = e, (m, c.name)
    print(f'orthogonality of the transcription: worst {worst:.2f} m u at {at}')
    assert 2 * worst <= BAR_ORTH <= 3 * worst, (worst, at)


@pytest.mark.parametrize('mutate', MUTATIONS)
def test_the_checker_has_teeth(mutate):
    """each wrong kernel is rejected on at least one catalogue input (and the right one on none: the tests above)"""
    rejected = []
    for m in (7, 8, 24):
        for c in cases(m):
            try:
                accept(c.G, spectrum(c.G, m, mutate=mutate), m, c.exact)
            except AssertionError as e:
                rejected.append((m, c.name, e.args[0][0] if isinstance(e.args[0], tuple) else e.args[0]))
    print(f'{mutate}: rejected on {len(rejected)} inputs, e.g. {rejected[:4]}')
    assert rejected
    if mutate == 'pad':
        assert all(m == 7 for m, _, _ in rejected)         # an even m has no pad row
    if mutate == 'expvar_noclamp':
        assert {n for _, n, _ in rejected} >= {'indefinite'}
    if mutate == 'tie':
        assert ('diagonal repeats' in {n for _, n, _ in rejected})


@pytest.mark.parametrize('m', [4, 5, 24])
def test_underflow_trigger_breaks_the_old_formula_only(m):
    G = case(m, 'underflow trigger').G
    c, s = rotation(np.array([1.0]), np.array([1.0]), np.array([1e-200]), fixed=False)
    assert np.isnan(c[0]) and np.isnan(s[0])
    old = spectrum(G, m, fixed=False)
    assert all(np.isnan(old[k]).all() for k in ('lam', 'S', 'V', 'W', 'Ar'))
    c, s = rotation(np.array([1.0]), np.array([1.0]), np.array([1e-200]))
    assert c[0] == s[0] and abs(c[0] - np.sqrt(0.5)) <= U     # w == 0: t = 1
    new = spectrum(G, m)
    accept(G, new, m)
    assert np.sum(np.abs(new['lam'] - 1.0) <= 4 * m * U * norm2(G)) == 2


def test_rotation_is_finite_and_orthogonal_over_the_whole_range():
    """every finite input with |a_pq| > 1e-300, squares that underflow or overflow included; inputs whose h2 stays in range take
    the old formula bit for bit"""
    rng = np.random.default_rng(5)
    mag = 10.0 ** rng.uniform(-299.5, 160, (3, 4000))
    app, aqq, apq = mag * rng.choice([-1.0, 1.0], mag.shape)
    app[:500] = aqq[:500]                                   # w == 0
    c, s = rotation(app, aqq, apq)
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(s))
    assert np.max(np.abs(c * c + s * s - 1.0)) <= 4 * U
    with np.errstate(all='ignore'):
        h2 = (aqq - app) ** 2 + (2 * apq) ** 2
    ok = (h2 >= TINY) & (h2 < np.inf)
    c0, s0 = rotation(app, aqq, apq, fixed=False)
    assert ok.sum() > 1000 and (~ok).sum() > 100
    assert np.array_equal(c[ok], c0[ok]) and np.array_equal(s[ok], s0[ok])
    # ... and it annihilates: the rotated off-diagonal entry is small against the block
    x = c * s * (app - aqq) + (c * c - s * s) * apq
    assert np.all(np.abs(x) <= 8 * U * (np.abs(app) + np.abs(aqq) + np.abs(apq)))


def test_sort_is_a_permutation_with_nan():
    for lam in ([1.0, np.nan, 2.0], [np.nan] * 5, [3.0, 3.0, np.nan, -1.0, np.nan, 3.0], [0.0, -0.0, np.inf, -np.inf, np.nan]):
        lam = np.array(lam)
        order = sort_order(lam)
        assert sorted(order) == list(range(len(lam))), (lam, order)
        nn = lam[order][~np.isnan(lam[order])]
        assert np.all(np.isnan(lam[order][:np.isnan(lam).sum()])) and np.all(np.diff(nn) <= 0)   # NaN first, then descending
    assert sorted(sort_order(np.array([1.0, np.nan, 2.0]), total=False)) != [0, 1, 2]              # the old rule: two share a rank
    lam = np.array([2.0, 5.0, 2.0, 7.0, 5.0])
    assert np.array_equal(sort_order(lam), sort_order(lam, total=False)) and list(sort_order(lam)) == [3, 1, 4, 0, 2]

"""csrc/measure.hip (Theta = C Ur, cnt = C X_cnt, scl = C X_scl for a CSR matrix C) and its sampled consumers: the cases, the
longdouble reference, the bars and the checker that both this file and tests/test_measure_gpu.py use, and the CPU-side
conditions on them.  Nothing here needs a GPU.

Reference (ref_measure): per row of C, the plain sum over the stored entries whose column lies in the shard, every product and
every sum in np.longdouble, and beside each sum the sum of the absolute terms T (T[i, k] = sum_e |v_e| |U[col_e, k]|, the same
for cnt and scl).  An f32 basis is widened as it is stored.

Bar (measure_bar), derived from the kernel and not from any result: the four waves of a workgroup take the stored entries of
a row round robin, so each wave runs a chain of at most ceil(L / 4) fused multiply-adds onto 0.0, one rounding each, every
intermediate bounded by the wave's share of T; the four partial sums are added in a fixed order onto 0.0, three more
roundings; one more unit covers the reference (at most 2 L 2^-64 T of its own, a quarter of a unit at L = 257) and its
comparison in longdouble.  With u = 2^-53:

    |got - ref| <= (ceil(L / 4) + 4) u T,     L = ALL stored entries of the row (a skipped entry keeps its wave slot).

Where T == 0 (an empty row, a row with no entry in the shard, a row of stored zeros) the result is exactly 0, and a one-hot
row with the value 1.0 is an exact gather: Theta[i] == Ur[col], cnt[i] == rowmean[col], scl[i] == scale[feature of col].

tests/numpy_engine.NumpyEngine.measure_csr adds a row's terms one after the other with a separately rounded product, for
which the bar is no worst-case bound (that would be 2 L u T); it passes because rounding errors do not all point the same
way -- its worst ratio is printed.  The bar is a bound for the kernel, which is what it is for.

Wrong twins: TwinEngine restates NumpyEngine.measure_csr (bit for bit, asserted) with seven switchable defects, one per
subclass -- the mistakes a measure kernel can make at the places the cases aim at.  Each must be rejected by the checker on a
named case.  No wrong kernel is built or run on a GPU.

Sampled reconstruct (ref_reconstruct, reconstruct_bar): x[p, i] = rs_i (u_i . a_p) + mu_i in longdouble; the bar is
(r + 4) u (|rs_i| sum_k |a_pk u_ik| + |mu_i|): an r-term dot product in any order (r roundings at most), the fused
scale-and-add (one), the accumulate pass of a second column group (one), and the reference."""
import collections
import math

import numpy as np
import pytest
import torch

from tests.numpy_engine import NumpyEngine

LD = np.longdouble
U53 = 2.0 ** -53

N_POINTS, N_FEATURES = 200, 3
N = N_POINTS * N_FEATURES
SCALE = np.array([0.5, 20.0, 3e-3])
WHOLE = (0, N)
SHARDS = [(0, 250), (250, 100), (350, 250)]                   # (row0, n_rows): both cuts lie inside a feature
L_LIST = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257]         # one, two and many rounds of the four waves, ragged last rounds
WIDTHS_F64 = [0, 1, 2, 63, 64, 65, 127, 128, 129, 256, 257]   # second accumulator from 65, second column group from 129
WIDTHS_F32 = [1, 65, 128, 257]
R_MAX = 257


# ------------------------------------------------------------------------------------------------ inputs
def _magnitudes(rng, shape, lo, hi):
    return 10.0 ** rng.uniform(lo, hi, shape)


_rng = np.random.default_rng(20261020)
BASIS = _rng.standard_normal((N, R_MAX)) * _magnitudes(_rng, (N, 1), -3, 3)      # rows of very different magnitude
BASIS32 = BASIS.astype(np.float32)
ROWMEAN = 10 * _rng.standard_normal(N)
del _rng


def basis(r, f32=False):
    """the first r columns of the one basis every case shares (None for r = 0), contiguous"""
    return None if r == 0 else np.ascontiguousarray((BASIS32 if f32 else BASIS)[:, :r])


Rows = collections.namedtuple('Rows', 'indptr indices vals names')


def build_rows():
    """The hand-built C: -> Rows(indptr, indices, vals, names), names[i] says what row i is there for."""
    rng = np.random.default_rng(7)
    rows = []

    def val(k):
        return rng.standard_normal(k) * _magnitudes(rng, k, -2, 2)

    def add(name, cols, vals=None):
        cols = np.asarray(cols, dtype=np.int64)
        rows.append((name, cols, val(len(cols)) if vals is None else np.asarray(vals, dtype=np.float64)))

    add('empty first', [])
    for L in L_LIST[1:]:                                      # anywhere in the matrix: these straddle every shard cut
        add(f'L={L}', np.sort(rng.choice(N, L, replace=False)))
    for col in (0, N_POINTS - 1, N_POINTS, 2 * N_POINTS - 1, 2 * N_POINTS, N - 1):
        add(f'one-hot feature edge {col}', [col], [1.0])
    for col in sorted({c for row0, n_rows in SHARDS for c in (row0 - 1, row0, row0 + n_rows - 1, row0 + n_rows)
                       if 0 <= c < N} - {0, N - 1}):
        add(f'one-hot shard edge {col}', [col], [1.0])
    add('empty middle', [])
    add('same column three times', [123, 123, 123])
    add('same column, values cancel', [377, 377], [2.5, -2.5])
    add('descending columns', [590, 401, 333, 260, 120, 3])
    add('zeros and negatives', [10, 210, 410, 411, 599], [0.0, -0.0, -1.5, -2e-2, -7.0])
    add('stored zeros only', [5, 255, 455], [0.0, -0.0, 0.0])
    add('feature 1 only', np.sort(rng.choice(np.arange(N_POINTS, 2 * N_POINTS), 6, replace=False)))
    add('all three features', [17, 180, 222, 391, 405, 577])
    for row0, n_rows in SHARDS:                               # several entries, all of them inside one shard
        add(f'inside shard {row0}', np.sort(rng.choice(np.arange(row0, row0 + n_rows), 5, replace=False)))
    for L in (5, 9, 65):                                      # ragged rounds once more, columns in no order
        add(f'L={L} unsorted', rng.permutation(rng.choice(N, L, replace=False)))
    for L in (1, 2, 3, 4, 7, 8):                              # short rows inside the narrowest shard; the single entry is not 1.0
        add(f'L={L} inside shard 250', np.sort(rng.choice(np.arange(250, 350), L, replace=False)))
    add('L=6 around the cuts', [248, 249, 250, 349, 350, 351])
    add('empty last', [])
    # the row before the last one is not empty and has a non-zero cnt: a stale cnt would show
    indptr = np.concatenate([[0], np.cumsum([len(c) for _, c, _ in rows])]).astype(np.int64)
    indices = np.concatenate([c for _, c, _ in rows]).astype(np.int64)
    vals = np.concatenate([v for _, _, v in rows]).astype(np.float64)
    return Rows(indptr, indices, vals, [n for n, _, _ in rows])


ROWS = build_rows()


def take_rows(rows, order):
    """the rows `order` of a Rows, in that order"""
    parts = [slice(rows.indptr[i], rows.indptr[i + 1]) for i in order]
    indptr = np.concatenate([[0], np.cumsum([p.stop - p.start for p in parts])]).astype(np.int64)
    return Rows(indptr, np.concatenate([rows.indices[p] for p in parts] + [np.zeros(0, np.int64)]),
                np.concatenate([rows.vals[p] for p in parts] + [np.zeros(0)]), [rows.names[i] for i in order])


def public_rows():
    """About twenty rows of the builder that mean the same in every form a caller may hand over (ndarray, scipy.sparse,
    DeviceCSR): no column stored twice, no stored zero, columns ascending in every row."""
    keep = []
    for i, name in enumerate(ROWS.names):
        lo, hi = ROWS.indptr[i], ROWS.indptr[i + 1]
        cols, v = ROWS.indices[lo:hi], ROWS.vals[lo:hi]
        if hi - lo <= 65 and len(set(cols.tolist())) == len(cols) and np.all(v != 0) and np.all(np.diff(cols) > 0):
            keep.append(i)
    keep = keep[:1] + keep[1:-1:2][:18] + keep[-1:]           # the empty first and last rows stay
    return take_rows(ROWS, keep)


def row_kinds(rows, row0, n_rows):
    """-> 'inside' / 'outside' / 'straddle' / 'empty' per row, for the shard [row0, row0 + n_rows)"""
    out = []
    for i in range(len(rows.indptr) - 1):
        c = rows.indices[rows.indptr[i]:rows.indptr[i + 1]]
        m = (c >= row0) & (c < row0 + n_rows)
        out.append('empty' if len(c) == 0 else 'inside' if m.all() else 'outside' if not m.any() else 'straddle')
    return out


# ------------------------------------------------------------------------------------------------ reference and bar
def ref_measure(indptr, indices, vals, U, rowmean, scale, n_points, row0, n_rows):
    """U (n_rows, r) or None and rowmean (n_rows,): the shard's block; indices: global columns.
    -> dict of longdouble arrays Theta, cnt, scl with the sums of absolute terms T_Theta, T_cnt, T_scl, the stored entries per
    row L, and exact: the rows whose result is an exact gather (one stored entry of value 1.0)"""
    s = len(indptr) - 1
    r = 0 if U is None else U.shape[1]
    assert rowmean.shape == (n_rows,) and (U is None or U.shape[0] == n_rows)
    Uw = np.zeros((n_rows, 0), dtype=LD) if U is None else np.asarray(U).astype(LD)
    mu, sc = np.asarray(rowmean).astype(LD), np.asarray(scale).astype(LD)
    out = {k: np.zeros((s, r) if 'Theta' in k else s, dtype=LD) for k in ('Theta', 'T_Theta', 'cnt', 'T_cnt', 'scl', 'T_scl')}
    for i in range(s):
        cols, v = indices[indptr[i]:indptr[i + 1]], vals[indptr[i]:indptr[i + 1]].astype(LD)
        for c, ve in zip(cols, v):                            # one entry after the other: plain sums
            if not row0 <= c < row0 + n_rows:
                continue
            f = min(int(c) // n_points, len(sc) - 1)
            for key, term in (('Theta', ve * Uw[c - row0]), ('cnt', ve * mu[c - row0]), ('scl', ve * sc[f])):
                out[key][i] += term
                out['T_' + key][i] += np.abs(term)
    out['L'] = np.diff(indptr)
    out['exact'] = np.array([out['L'][i] == 1 and vals[indptr[i]] == 1.0 for i in range(s)], dtype=bool)
    return out


def measure_bar(L, T):
    """(ceil(L / 4) + 4) u T, entrywise; L per row"""
    steps = (np.ceil(np.asarray(L) / 4) + 4).astype(LD)
    return (steps[:, None] if np.ndim(T) == 2 else steps) * LD(U53) * T


def check_measure(got, ref, tag=''):
    """got = (Theta or None, cnt, scl or None) float64 host arrays.  Asserts the contract of the module docstring against
    ref_measure's dict and returns the worst error / bar ratio."""
    worst = 0.0
    for key, g in zip(('Theta', 'cnt', 'scl'), got):
        want, T = ref[key], ref['T_' + key]
        if g is None:
            assert key != 'cnt' and (key == 'scl' or want.shape[1] == 0), (tag, key, 'missing output')
            continue
        assert g.dtype == np.float64 and g.shape == want.shape, (tag, key, g.dtype, g.shape, want.shape)
        assert np.all(np.isfinite(g)), (tag, key, 'not finite')
        zero = T == 0
        assert np.all(g[zero] == 0), (tag, key, 'T == 0 but the result is not 0, rows', np.unique(np.nonzero(~(g == 0) & zero)[0]))
        ex = ref['exact']
        assert np.array_equal(g[ex], want[ex].astype(np.float64)), (
            tag, key, 'a one-hot row of value 1.0 is not an exact gather, rows', np.nonzero(ex)[0][np.any(
                (g[ex] != want[ex].astype(np.float64)).reshape(int(ex.sum()), -1), axis=1)])
        bar = measure_bar(ref['L'], T)
        err = np.abs(g.astype(LD) - want)
        ratio = np.where(zero, 0, err / np.where(zero, 1, bar))
        w = float(ratio.max(initial=0))
        assert w <= 1.0, (tag, key, 'error / bar', w, 'at', np.unravel_index(np.argmax(ratio), ratio.shape))
        worst = max(worst, w)
    return worst


# ------------------------------------------------------------------------------------------------ one call
def host(eng, t):
    return None if t is None else np.array(eng.to_host(t.contiguous()))


def upload_csr(eng, rows):
    t = eng.torch
    return (eng.to_device(rows.indptr, dtype=t.int64), eng.to_device(rows.indices, dtype=t.int64), eng.to_device(rows.vals))


def measure(eng, rows, U, pad=0, scl=True, shard=WHOLE, twice=False):
    """One eng.measure_csr call on the shard's block.  U: (N, r) host array, float64 or float32, or None (r = 0).  pad > 0: the
    basis is a column view of a matrix pad columns wider whose other columns hold NaN.  The block and its rowmean are row
    slices of the whole tensors.  twice: call again and compare the bits.  -> (Theta or None, cnt, scl or None) on the host"""
    t = eng.torch
    row0, n_rows = shard
    ip, ix, v = upload_csr(eng, rows)
    Ud = None
    if U is not None:
        dt = t.float32 if U.dtype == np.float32 else t.float64
        Ud = eng.to_device(U, dtype=dt)
        if pad:
            wide = t.full((N, U.shape[1] + pad), float('nan'), dtype=dt, device=eng.device)
            wide[:, :U.shape[1]] = Ud
            Ud = wide[:, :U.shape[1]]
            assert Ud.stride(0) == U.shape[1] + pad
        Ud = Ud[row0:row0 + n_rows]
    mu = eng.to_device(ROWMEAN)[row0:row0 + n_rows]
    kw = dict(scale=eng.to_device(SCALE), n_points=N_POINTS) if scl else {}
    runs = []
    for _ in range(2 if twice else 1):
        out = eng.measure_csr(ip, ix, v, Ud, row0, mu, **kw)
        assert len(out) == (3 if scl else 2) and (out[0] is None) == (U is None)
        runs.append(tuple(host(eng, x) for x in out) + ((None,) if not scl else ()))
    if twice:
        for a, b in zip(*runs):
            assert (a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())
    return runs[0]


def reference(rows, U, shard=WHOLE):
    row0, n_rows = shard
    return ref_measure(rows.indptr, rows.indices, rows.vals, None if U is None else U[row0:row0 + n_rows],
                       ROWMEAN[row0:row0 + n_rows], SCALE, N_POINTS, row0, n_rows)


Case = collections.namedtuple('Case', 'name r f32 pad scl shard')


def measure_cases():
    """every call of the first part of tests/test_measure_gpu.py"""
    out = []
    for r in WIDTHS_F64:
        for pad in (0, 3) if r else (0,):
            for scl in (True, False):
                out.append(Case(f'r={r} f64{" view" if pad else ""}{"" if scl else " no scl"}', r, False, pad, scl, WHOLE))
    for r in WIDTHS_F32:
        for scl in (True, False):
            out.append(Case(f'r={r} f32{"" if scl else " no scl"}', r, True, 0, scl, WHOLE))
    for shard in SHARDS:
        for r in (0, 5, 129):
            out.append(Case(f'shard {shard[0]}+{shard[1]} r={r}', r, False, 0, True, shard))
    return out


CASES = measure_cases()
_REF = {}


def case_reference(case):
    """computed once per (r, storage, shard) and shared"""
    key = (case.r, case.f32, case.shard)
    if key not in _REF:
        _REF[key] = reference(ROWS, basis(case.r, case.f32), case.shard)
    return _REF[key]


def run_case(eng, case, twice=False):
    """-> (got, worst error / bar)"""
    got = measure(eng, ROWS, basis(case.r, case.f32), case.pad, case.scl, case.shard, twice)
    return got, check_measure(got, case_reference(case), case.name)


# ------------------------------------------------------------------------------------------------ sampled reconstruct
def ref_reconstruct(U, A, rs, mu):
    """U (s, r), A (n_p, r), rs (s,), mu (s,) -> x (n_p, s) = rs_i (u_i . a_p) + mu_i in longdouble, and the scale
    |rs_i| sum_k |a_pk u_ik| + |mu_i| of every entry"""
    Uw, Aw, rsw, muw = (np.asarray(x).astype(LD) for x in (U, A, rs, mu))
    x = np.zeros((A.shape[0], U.shape[0]), dtype=LD)
    T = np.zeros_like(x)
    for k in range(U.shape[1]):                               # column by column: plain longdouble sums
        term = Aw[:, k, None] * Uw[None, :, k]
        x += term
        T += np.abs(term)
    return rsw * x + muw, np.abs(rsw) * T + np.abs(muw)


def reconstruct_bar(r, T):
    return (r + 4) * LD(U53) * T


def check_reconstruct(got, want, T, r, tag=''):
    assert got.dtype == np.float64 and got.shape == want.shape and np.all(np.isfinite(got)), tag
    bar = reconstruct_bar(r, T)
    zero = bar == 0
    err = np.abs(got.astype(LD) - want)
    assert np.all(err[zero] == 0), tag
    w = float(np.where(zero, 0, err / np.where(zero, 1, bar)).max(initial=0))
    assert w <= 1.0, (tag, 'error / bar', w)
    return w


def reconstruct_inputs(s, r, n_p, f32=False, seed=0):
    """rows of very different magnitude, a per-row scale of either sign, a centre that dominates some rows and not others"""
    rng = np.random.default_rng([s, r, n_p, seed])
    U = rng.standard_normal((s, r)) * _magnitudes(rng, (s, 1), -3, 3)
    if f32:
        U = U.astype(np.float32)
    A = rng.standard_normal((n_p, r)) * _magnitudes(rng, (n_p, 1), -1, 1)
    rs = rng.standard_normal(s) * _magnitudes(rng, s, -2, 2)
    mu = 10 * rng.standard_normal(s) * (rng.random(s) < 0.8)
    return U, A, rs, mu


# ------------------------------------------------------------------------------------------------ wrong twins
class TwinEngine(NumpyEngine):
    """NumpyEngine.measure_csr once more, with one switchable defect"""
    defect = None

    def measure_csr(self, indptr, indices, vals, Ur, row0, rowmean, scale=None, n_points=0):
        ip, ix, v = indptr.numpy(), indices.numpy(), vals.numpy()
        s, n, r = len(ip) - 1, rowmean.shape[0], (Ur.shape[1] if Ur is not None else 0)
        Theta, cnt, scl = np.zeros((s, r)), np.zeros(s), np.zeros(s)
        U, mu = (self._w(Ur) if Ur is not None else np.zeros((n, 0))), rowmean.numpy()
        d = self.defect
        for i in range(s):
            ents = list(range(ip[i], ip[i + 1]))
            if d == 'drops the last entry of rows with L % 4 == 1' and len(ents) % 4 == 1:
                ents = ents[:-1]
            if d == 'keeps only the first of duplicated columns':
                ents = [e for k, e in enumerate(ents) if ix[e] not in ix[ents[:k]]]
            if d == 'cnt of the previous row for an empty row' and not ents and i > 0:
                cnt[i] = cnt[i - 1]
            for e in ents:
                col = ix[e] - row0
                top = n + 1 if d == '> instead of >= at the upper shard edge' else n
                if 0 <= col < top:
                    col = min(col, n - 1)                     # the defective edge reads what lies behind the block
                    Theta[i] += v[e] * U[col]
                    cnt[i] += v[e] * mu[col]
                    if scale is not None:
                        g = col if d == 'feature from the local column' else ix[e]
                        scl[i] += v[e] * scale.numpy()[min(g // n_points, scale.shape[0] - 1)]
        if d == 'ignores basis columns >= 64':
            Theta[:, 64:] = 0
        if d == 'column group 2 written over group 1' and r > 128:
            Theta[:, :r - 128], Theta[:, 128:] = Theta[:, 128:].copy(), 0
        out = (torch.from_numpy(Theta) if Ur is not None else None, torch.from_numpy(cnt))
        return out if scale is None else out + (torch.from_numpy(scl),)


# defect -> a case that must reject it (every case that does is printed)
TWINS = {
    'drops the last entry of rows with L % 4 == 1': 'r=1 f64',
    'ignores basis columns >= 64': 'r=65 f64',
    'column group 2 written over group 1': 'r=129 f64',
    '> instead of >= at the upper shard edge': 'shard 0+250 r=5',
    'feature from the local column': 'shard 250+100 r=0',
    'keeps only the first of duplicated columns': 'r=0 f64',
    'cnt of the previous row for an empty row': 'r=2 f64 view no scl',
}
TWIN_CLASSES = {d: type('Twin' + str(k), (TwinEngine,), {'defect': d}) for k, d in enumerate(TWINS)}


# ------------------------------------------------------------------------------------------------ host tests
def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_conditions_on_the_rows():
    L = np.diff(ROWS.indptr)
    assert 40 <= len(L) <= 50 and L[0] == 0 and L[-1] == 0 and L[-2] > 0
    assert sorted(set(L_LIST) - set(L.tolist())) == []
    assert ROWS.indices.min() == 0 and ROWS.indices.max() == N - 1
    onehot = {int(ROWS.indices[ROWS.indptr[i]]) for i in range(len(L)) if L[i] == 1 and ROWS.vals[ROWS.indptr[i]] == 1.0}
    assert {0, N_POINTS - 1, N_POINTS, 2 * N_POINTS - 1, 2 * N_POINTS, N - 1} <= onehot
    for row0, n_rows in SHARDS:
        assert row0 % N_POINTS or (row0 + n_rows) % N_POINTS                      # a cut inside a feature
        assert {c for c in (row0 - 1, row0, row0 + n_rows - 1, row0 + n_rows) if 0 <= c < N} <= onehot
        kinds = row_kinds(ROWS, row0, n_rows)
        several = [k for k, l in zip(kinds, L) if l > 1]
        assert {'inside', 'outside', 'straddle'} <= set(several), (row0, n_rows)
    assert sum(n for _, n in SHARDS) == N and [r0 for r0, _ in SHARDS] == [0, 250, 350]
    by_name = dict(zip(ROWS.names, range(len(L))))
    c = ROWS.indices[ROWS.indptr[by_name['same column three times']]:][:3]
    assert len(set(c.tolist())) == 1
    lo = ROWS.indptr[by_name['descending columns']]
    assert np.all(np.diff(ROWS.indices[lo:lo + 6]) < 0)
    lo = ROWS.indptr[by_name['zeros and negatives']]
    z = ROWS.vals[lo:lo + 5]
    assert z[0] == 0 and not np.signbit(z[0]) and z[1] == 0 and np.signbit(z[1]) and np.all(z[2:] < 0)
    lo = ROWS.indptr[by_name['feature 1 only']]
    assert set((ROWS.indices[lo:lo + 6] // N_POINTS).tolist()) == {1}
    lo = ROWS.indptr[by_name['all three features']]
    assert set((ROWS.indices[lo:lo + 6] // N_POINTS).tolist()) == {0, 1, 2}
    mag = np.abs(BASIS).max(axis=1)
    assert mag.max() / mag.min() > 1e4                                            # what makes an entrywise bar matter


def test_conditions_on_the_public_rows():
    pub = public_rows()
    L = np.diff(pub.indptr)
    assert 15 <= len(L) <= 25 and L[0] == 0 and L[-1] == 0 and L.max() >= 9 and np.all(pub.vals != 0)
    for i in range(len(L)):
        assert np.all(np.diff(pub.indices[pub.indptr[i]:pub.indptr[i + 1]]) > 0)


def test_cases_cover_what_the_kernel_branches_on():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.r for c in CASES if not c.f32 and c.shard == WHOLE} == set(WIDTHS_F64)
    assert {c.r for c in CASES if c.f32} == set(WIDTHS_F32)
    assert all(any(c.r == r and c.pad == p and c.scl == q for c in CASES) for r in WIDTHS_F64[1:] for p in (0, 3) for q in (True, False))
    assert {c.shard for c in CASES} == set(SHARDS) | {WHOLE}
    assert set(TWINS.values()) <= set(names)


def test_numpy_engine_passes_every_case():
    eng = NumpyEngine()
    worst = {c.name: run_case(eng, c, twice=True)[1] for c in CASES}
    print('measure, NumpyEngine: worst error / bar over', len(CASES), 'cases:', f'{max(worst.values()):.3f}', 'in',
          max(worst, key=worst.get))
    assert max(worst.values()) <= 1.0


def test_twin_without_a_defect_is_the_numpy_engine():
    a, b = NumpyEngine(), TwinEngine()
    for c in CASES:
        x, y = (measure(e, ROWS, basis(c.r, c.f32), c.pad, c.scl, c.shard) for e in (a, b))
        assert all((p is None and q is None) or p.tobytes() == q.tobytes() for p, q in zip(x, y)), c.name


@pytest.mark.parametrize('defect', list(TWINS))
def test_checker_rejects_the_wrong_twin(defect):
    eng = TWIN_CLASSES[defect]()
    assert isinstance(eng, NumpyEngine) and eng.defect == defect
    rejected = []
    for c in CASES:
        try:
            run_case(eng, c)
        except AssertionError:
            rejected.append(c.name)
    print(f'wrong twin "{defect}": rejected on {len(rejected)} of {len(CASES)} cases, first {rejected[:3]}')
    assert TWINS[defect] in rejected, (defect, TWINS[defect], rejected)


def test_no_stored_entries_numpy_engine():
    eng, t = NumpyEngine(), torch
    for s, r in ((1, 0), (5, 3)):
        Th, cnt, scl = eng.measure_csr(t.zeros(s + 1, dtype=t.int64), t.zeros(0, dtype=t.int64), t.zeros(0, dtype=t.float64),
                                       None if r == 0 else eng.to_device(basis(r)), 0, eng.to_device(ROWMEAN),
                                       scale=eng.to_device(SCALE), n_points=N_POINTS)
        assert (Th is None) == (r == 0) and (r == 0 or (Th.shape == (s, r) and not Th.any()))
        assert cnt.shape == (s,) and scl.shape == (s,) and not cnt.any() and not scl.any()


def test_rows_do_not_interact_numpy_engine():
    eng = NumpyEngine()
    order = np.random.default_rng(3).permutation(len(ROWS.names))
    U = basis(65)
    a, b = measure(eng, ROWS, U), measure(eng, take_rows(ROWS, order), U)
    assert all(x[order].tobytes() == y.tobytes() for x, y in zip(a, b))


def test_reconstruct_reference_against_numpy_engine():
    eng = NumpyEngine()
    worst = 0.0
    for s, r, n_p, f32 in ((1, 1, 1, False), (17, 13, 16, False), (65, 48, 17, True), (130, 129, 3, False)):
        U, A, rs, mu = reconstruct_inputs(s, r, n_p, f32)
        want, T = ref_reconstruct(U, A, rs, mu)
        got = eng.reconstruct(eng.to_device(U, dtype=torch.float32 if f32 else None), 0, s, 1, eng.to_device(mu),
                              eng.to_device(np.ones(1)), eng.to_device(A), rowscale=eng.to_device(rs))
        worst = max(worst, check_reconstruct(host(eng, got), want, T, r, (s, r, n_p)))
        with pytest.raises(AssertionError):                   # one entry moved by two bars is noticed
            bad = host(eng, got)
            bad[-1, -1] += 2 * float(reconstruct_bar(r, T)[-1, -1]) + np.spacing(bad[-1, -1])
            check_reconstruct(bad, want, T, r)
    print(f'sampled reconstruct, NumpyEngine: worst error / bar {worst:.3f}')

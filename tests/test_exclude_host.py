"""Distance exclusion and masking of the placement (csrc/qr_pivot.hip: qr_exclude_kernel, the within() test inside the
candidate steps, mask_rows_kernel) on the CPU: literal restatements of the reference's expressions, and the cases on which
the comparison `|p - c| < d_min` is decided by the last bit -- structured lattices with d_min a distance NumPy itself
produces between two of their points.  The reference keeps a row when np.linalg.norm(p_sensor - xyz, axis=1) >= d_min
(:647-649, :686-688): every square rounded, the squares added in index order, a correctly rounded square root.  A sum of
squares accumulated with fused multiply-adds rounds once less and puts some points of the d_min sphere on the other side;
fused_dist emulates that arithmetic exactly and serves ONLY to prove that a case has such points -- the expected results
come from NumPy's expression alone.  tests/test_exclude_gpu.py runs the cases built here on the HIP engine; this file runs
them on the NumPy double."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from openmeasure_amd._placement import pivot_loop
from openmeasure_amd.sparse_sensing import SPR
from oracle import spr_oracle as orc
from tests.numpy_engine import NumpyEngine
from tests.test_design_host import DesignEngine

QR_BATCH = 16                                     # spr_qr_batch() of the library (the GPU tests assert it)


# ---- restatements -------------------------------------------------------------------------------------------------------
def np_exclude(nrm, row0, n_points, mask, xyz, picks, d_min):
    """What qr_exclude leaves in nrm (local rows row0 .. row0 + len(nrm) of a feature-major matrix): rows outside `mask`
    (one entry per local row) and rows closer than d_min to the cell of a pick (global rows; < 0 = no pick) are -1, by the
    reference's literal expression; every other entry is untouched."""
    out = np.array(nrm, dtype=np.float64, copy=True)
    gone = np.zeros(out.shape[0], dtype=bool)
    if mask is not None:
        gone |= ~np.asarray(mask, dtype=bool)
    if xyz is not None:
        pos = xyz[(row0 + np.arange(out.shape[0])) % n_points]
        for g in picks:
            if g >= 0:
                gone |= np.linalg.norm(xyz[g % n_points] - pos, axis=1) < d_min
    out[gone] = -1.0
    return out


def np_mask_rows(U, mask):
    """Ur[~mask, :] = 0 (:737-738)"""
    out = np.array(U, copy=True)
    out[~np.asarray(mask, dtype=bool), :] = 0
    return out


def fused_dist(p, c):
    """sqrt of d2 = fma(t, t, d2), t = c[d] - p[d] in index order: each product added to the running sum and rounded ONCE
    (exact rational arithmetic, one rounding to double per step), then a correctly rounded root.  Not a reference."""
    d2 = 0.0
    for a, b in zip(p, c):
        t = float(b) - float(a)
        d2 = float(Fraction(t) * Fraction(t) + Fraction(d2))
    return float(np.sqrt(d2))


# ---- lattices -----------------------------------------------------------------------------------------------------------
# np.linspace(0, 1, m) per axis (spacing 1/40, 1/20: not dyadic) and a d_min NumPy realises between two lattice points:
# 2-D the ring of the offsets (3, 8); 3-D three cells, the ring of (3, 0, 0) and (2, 2, 1)
LATTICES = {2: (41, 0.21360009363293833), 3: (21, 0.15)}
PLANT_HINT = {2: 870, 3: 1440}                   # where the search for a planted centre starts (it wraps around)


@functools.lru_cache(maxsize=None)
def lattice(dim):
    m, d_min = LATTICES[dim]
    ax = np.linspace(0.0, 1.0, m)
    xyz = np.ascontiguousarray(np.stack(np.meshgrid(*[ax] * dim, indexing='ij'), -1).reshape(-1, dim))
    xyz.setflags(write=False)
    return xyz, d_min


def ring_flips(xyz, centre, d_min):
    """Cells on the d_min sphere of `centre` that the fused sum decides differently from NumPy ->
    (fused < d_min <= numpy: a fused kernel excludes them, the reference keeps them,
     numpy < d_min <= fused: a fused kernel keeps them, the reference excludes them), with NumPy's distances."""
    d = np.linalg.norm(xyz[centre] - xyz, axis=1)
    near = np.flatnonzero(np.abs(d - d_min) <= 8 * np.spacing(d_min))
    fd = {int(j): fused_dist(xyz[j], xyz[centre]) for j in near}
    inside = [j for j in fd if fd[j] < d_min <= d[j]]
    outside = [j for j in fd if d[j] < d_min <= fd[j]]
    return inside, outside, d


@functools.lru_cache(maxsize=None)
def lattice_case(dim, n_centres=QR_BATCH):
    """-> dict(xyz, n_points, d_min, centres, kept, gone): up to n_centres cells, at least 2.2 d_min apart (no ring point
    of one lies inside the sphere of another), whose rings hold cells of both kinds -- `kept`: the reference keeps them
    and the fused sum would exclude them, `gone`: the other way round."""
    xyz, d_min = lattice(dim)
    order = np.random.default_rng(dim).permutation(len(xyz))[:600]
    flips = {}

    def get(c):
        if c not in flips:
            inside, outside, d = ring_flips(xyz, c, d_min)
            flips[c] = (inside, outside, bool(np.any(d == d_min)))
        return flips[c]

    centres = []

    def fits(c):
        return all(np.linalg.norm(xyz[c] - xyz[o]) >= 2.2 * d_min for o in centres)

    for kind in (1, 0):                                      # the rarer kind first, then the other, then whatever fits
        c = next((int(c) for c in order if fits(c) and get(int(c))[kind]), None)
        assert c is not None, f'no centre with flips of kind {kind} on the {dim}-D lattice'
        if c not in centres:
            centres.append(c)
    for c in order:
        if len(centres) >= n_centres:
            break
        if int(c) not in centres and fits(c) and any(get(int(c))[:2]):
            centres.append(int(c))
    kept = sorted({j for c in centres for j in get(c)[0]})
    gone = sorted({j for c in centres for j in get(c)[1]})
    assert kept and gone and 2 <= len(centres) <= n_centres
    assert any(get(c)[2] for c in centres)                   # d_min is a distance NumPy produces on this lattice
    # the discrimination, pair by pair and on the rows: the literal expression against the fused emulation
    # (the literal expression with axis=1: the norm of ONE vector takes another route through NumPy, a dot product)
    dist = {c: np.linalg.norm(xyz[c] - xyz, axis=1) for c in centres}
    assert any(fused_dist(xyz[j], xyz[c]) < d_min <= dist[c][j] for c in centres for j in kept)
    assert any(dist[c][j] < d_min <= fused_dist(xyz[j], xyz[c]) for c in centres for j in gone)
    want = np_exclude(np.ones(len(xyz)), 0, len(xyz), None, xyz, centres, d_min)
    assert np.all(want[kept] == 1.0) and np.all(want[gone] == -1.0)
    return dict(xyz=xyz, n_points=len(xyz), d_min=d_min, centres=np.asarray(centres, dtype=np.int64), kept=kept, gone=gone)


# ---- planted placement --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_centre(dim):
    """The first cell (from PLANT_HINT on) whose ring holds both kinds of flipped cells, each decided by ONE ulp of d_min:
    kept cells at NumPy distance exactly d_min, gone cells at the double just below."""
    xyz, d_min = lattice(dim)
    n = len(xyz)
    below = np.nextafter(d_min, 0.0)
    for k in range(n):
        c = (PLANT_HINT[dim] + k) % n
        inside, outside, d = ring_flips(xyz, c, d_min)
        kept = [j for j in inside if d[j] == d_min]
        gone = [j for j in outside if d[j] == below]
        if kept and gone:
            return c, kept[:2], gone[:2]
    raise AssertionError(f'no centre with both kinds of flipped ring cells on the {dim}-D lattice')


@functools.lru_cache(maxsize=None)
def planted_case(dim, r, f32=False):
    """A basis (2 n_points, r) on the lattice, F = 2, on which the picks hang on the flipped ring cells: the centre row has
    by far the largest row variance, up to two `kept` and two `gone` ring cells of it carry the next-largest rows (each
    along a coordinate of its own, alternating features, amplitudes falling by 0.8), then two anchors far from everything;
    all other rows are 100 times smaller.  -> dict(Ur, xyz, n_points, F, d_min, centre, kept, gone, rows (the planted
    rows, centre first), s (the leading picks of the reference that are planted rows)); f32: Ur rounded to float32 storage."""
    xyz, d_min = lattice(dim)
    n_points, F = len(xyz), 2
    c, kept, gone = planted_centre(dim)
    cells = [c]
    for a, b in zip(gone, kept):                             # a gone cell first: were it kept, it would be the second pick
        cells += [a, b]
    cells += gone[len(kept):] + kept[len(gone):]
    far = np.argsort(-np.linalg.norm(xyz[c] - xyz, axis=1), kind='stable')
    for j in far:                                            # anchors: 2.5 d_min from every planted cell
        if len(cells) == 1 + len(kept) + len(gone) + 2:
            break
        if np.linalg.norm(xyz[cells] - xyz[j], axis=1).min() >= 2.5 * d_min:
            cells.append(int(j))
    assert len(cells) <= r - 1, 'more planted rows than noise-free GEM picks'
    rng = np.random.default_rng(100 * dim + r)
    Ur = 0.01 * rng.standard_normal((F * n_points, r))
    rows = []
    for i, cell in enumerate(cells):
        row = (i % F) * n_points + cell                      # alternating features: the cell counts, not the feature
        Ur[row, i] += 10.0 if i == 0 else 5.0 * 0.8 ** (i - 1)
        rows.append(row)
    if f32:
        Ur = Ur.astype(np.float32)
    Ur.setflags(write=False)
    case = dict(Ur=Ur, xyz=xyz, n_points=n_points, F=F, d_min=d_min, centre=c, kept=kept, gone=gone,
                rows=np.asarray(rows, dtype=np.int64))
    want, _ = oracle_picks(case, s=len(rows))                # the reference says how many of the planted rows it picks
    case['s'] = int(np.argmin(np.isin(want, rows))) if not np.isin(want, rows).all() else len(rows)
    return case


def oracle_picks(case, s=None, d_min=None, ridge=None):
    return orc.gem_pivots(np.asarray(case['Ur'], dtype=np.float64), s or case['s'], case['xyz'], case['F'], None,
                          case['d_min'] if d_min is None else d_min, ridge=ridge)


def check_planted(case):
    """The reference alone determines the picks, and they hang on the flipped cells: one ulp of d_min in the direction
    that inverts the kept cells (up) or the gone cells (down) changes the oracle's picks; every lead is above 1e-3."""
    want, lead = oracle_picks(case)
    assert lead.min() > 1e-3
    assert set(want.tolist()) <= set(case['rows'].tolist()) and want[0] == case['rows'][0]
    cells = set((want % case['n_points']).tolist())
    assert cells & set(case['kept']) and not cells & set(case['gone'])
    up, lead_up = oracle_picks(case, d_min=np.nextafter(case['d_min'], np.inf))
    down, lead_down = oracle_picks(case, d_min=np.nextafter(case['d_min'], 0.0))
    assert not np.array_equal(up, want) and not np.array_equal(down, want)
    assert set((down % case['n_points']).tolist()) & set(case['gone'])
    return want


def in_step_picks(eng, Ur_d, xyz_d, n_points, d_min, s):
    """qr_begin + pivot_loop as _placement_gem drives them (centring direction in slot 0) -> the s picks"""
    r = Ur_d.shape[1]
    st = eng.qr_begin(Ur_d, 0, s + 1)
    st['Q'][0] = r ** -0.5
    st['piv'][0] = -1
    eng.qr_refresh(st, 0, 1)
    pivot_loop(eng, st, s + 1, None, start=1, near=(xyz_d, n_points, float(d_min)))
    return np.asarray(eng.to_host(st['piv']))[1:].astype(np.int64)


def gem_spr(eng, case):
    n, r = case['Ur'].shape
    spr = SPR(np.zeros((n, r + 2)), case['F'], np.array(case['xyz']), engine=eng)
    spr.fit(basis=(np.array(case['Ur'], dtype=np.float64), np.eye(r + 2, r)))
    return spr


def gem_end_to_end(eng, case, n_sensors):
    """optimal_placement('gem', d_min) (an f32-stored basis: the public SPR.gem, which uploads it as float32 and runs the
    same placement) against gem_pivots on the stored values, up to the first lead below 1e-9; the planted picks lie before."""
    ridge = 1e-5 if n_sensors > case['Ur'].shape[1] - 1 else None
    want, lead = oracle_picks(case, s=n_sensors, ridge=ridge)
    spr = gem_spr(eng, case)
    if case['Ur'].dtype == np.float32:
        got = spr.gem(np.array(case['Ur']), n_sensors, None, case['d_min'], False)
    else:
        C = spr.optimal_placement(calc_type='gem', n_sensors=n_sensors, d_min=case['d_min'])
        assert C.shape == (n_sensors, case['Ur'].shape[0])
        got = spr.sensors_
    k = int(np.argmax(lead < 1e-9)) if (lead < 1e-9).any() else n_sensors
    planted = int(np.isin(want, case['rows']).sum())
    assert planted >= 3 and np.isin(want[:planted], case['rows']).all() and k >= planted
    print(f'gem: picks {np.asarray(got).tolist()} oracle {want.tolist()} compared up to {k}')
    np.testing.assert_array_equal(got[:k], want[:k])
    return got


def augment_picks(eng, case, d_min=None):
    """augment_placement from the centre row: D-optimal additions under a ridge, as many as the planted picks -> sensors,
    the smallest relative lead of an addition"""
    spr = gem_spr(eng, case)
    spr.augment_placement(case['s'], 'D', start=case['rows'][:1], d_min=case['d_min'] if d_min is None else d_min, ridge=1e-2)
    return spr.sensors_.copy(), float(spr.pivot_gap_[1:].min())


# ---- CPU checks ---------------------------------------------------------------------------------------------------------
def test_fused_dist_is_one_rounding_per_term():
    p, c = np.array([0.1, 0.7, 0.3]), np.array([0.25, 0.05, 0.9])
    t = c - p
    assert fused_dist(p[:1], c[:1]) == abs(t[0])             # one term: fma(t, t, 0) is the rounded square
    exact = sum(Fraction(float(x)) ** 2 for x in t)
    assert abs(Fraction(fused_dist(p, c)) ** 2 - exact) < exact * Fraction(1, 2 ** 50)


@pytest.mark.parametrize('dim', [2, 3])
def test_lattice_cases_discriminate(dim):
    case = lattice_case(dim)                                 # the builder asserts both kinds of flipped pairs
    xyz, d_min = case['xyz'], case['d_min']
    assert len(case['centres']) <= QR_BATCH
    d = np.linalg.norm(xyz[case['centres'], None, :] - xyz[None, case['centres'], :], axis=2)
    assert (d + 10.0 * np.eye(len(d))).min() >= 2.2 * d_min


def test_one_coordinate_cannot_flip():
    x = np.linspace(0.0, 1.0, 41)[:, None]
    for c in (0, 7, 20, 33):
        d = np.linalg.norm(x[c] - x, axis=1)
        assert all(fused_dist(x[j], x[c]) == d[j] for j in range(len(x)))


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('F,row0,extra', [(1, 0, 0), (3, None, 40)])
def test_numpy_engine_exclude_on_the_lattices(dim, F, row0, extra):
    case = lattice_case(dim)
    n_points = case['n_points']
    row0 = n_points + 13 if row0 is None else row0
    n = n_points + extra
    eng = NumpyEngine()
    rng = np.random.default_rng(dim)
    nrm = rng.random(n) + 0.5
    nrm[::7], nrm[3::11] = -1.0, 0.0
    mask = rng.random(n) < 0.8
    picks = case['centres'] + (F - 1) * n_points             # picks in the last feature: the cell counts
    st = dict(nrm=torch.from_numpy(nrm.copy()), n=n, row0=row0, Ur=torch.zeros((n, 1), dtype=torch.float64),
              piv=torch.from_numpy(picks))
    eng.qr_exclude(st, mask=torch.from_numpy(mask.astype(np.uint8)), xyz=torch.from_numpy(np.array(case['xyz'])),
                   n_points=n_points, j0=0, nq=len(picks), d_min=case['d_min'])
    want = np_exclude(nrm, row0, n_points, mask, case['xyz'], picks, case['d_min'])
    np.testing.assert_array_equal(st['nrm'].numpy().view(np.uint64), want.view(np.uint64))


def test_numpy_engine_mask_rows():
    rng = np.random.default_rng(3)
    for dtype in (np.float64, np.float32):
        U = rng.standard_normal((257, 3)).astype(dtype)
        mask = rng.random(257) < 0.5
        Ut = torch.from_numpy(U.copy())
        NumpyEngine().mask_rows(Ut, torch.from_numpy(mask.astype(np.uint8)))
        np.testing.assert_array_equal(Ut.numpy(), np_mask_rows(U, mask))


@pytest.mark.parametrize('dim', [2, 3])
def test_planted_case_hangs_on_the_flipped_cells(dim):
    check_planted(planted_case(dim, 8))


@pytest.mark.parametrize('dim,r', [(2, 8), (3, 8), (2, 131)])
def test_in_step_exclusion_through_the_numpy_engine(dim, r):
    case = planted_case(dim, r)
    want = check_planted(case)
    eng = NumpyEngine()
    got = in_step_picks(eng, eng.to_device(np.array(case['Ur'])), eng.to_device(np.array(case['xyz'])), case['n_points'],
                        case['d_min'], case['s'])
    np.testing.assert_array_equal(got, want)


class FusedExcludeEngine(NumpyEngine):
    """the double with the distance of a fused sum of squares: what the planted cases must tell from the reference"""

    @staticmethod
    def _exclude_near(st, xyz, n_points, picks, d_min):
        nrm = st['nrm'].numpy()
        cell = (st['row0'] + np.arange(st['n'])) % n_points
        for g in picks:
            if g >= 0:
                d = np.linalg.norm(xyz[cell] - xyz[g % n_points], axis=1)
                for i in np.flatnonzero(np.abs(d - d_min) <= 8 * np.spacing(d_min)):
                    d[i] = fused_dist(xyz[cell[i]], xyz[g % n_points])
                nrm[d < d_min] = -1.0


@pytest.mark.parametrize('dim', [2, 3])
def test_a_fused_sum_moves_the_planted_picks(dim):
    case = planted_case(dim, 8)
    want = check_planted(case)
    eng = FusedExcludeEngine()
    got = in_step_picks(eng, eng.to_device(np.array(case['Ur'])), eng.to_device(np.array(case['xyz'])), case['n_points'],
                        case['d_min'], case['s'])
    assert got[0] == want[0] and not np.array_equal(got, want)
    assert got[1] % case['n_points'] in case['gone']          # the cell the reference excludes is the fused sum's second pick


# (dim, f32-stored basis, sensors: None = the planted picks, 10 > r - 1 = 7: the ridge phase runs)
GEM_CASES = [(2, False, None), (3, False, None), (2, True, None), (3, True, None), (3, False, 10)]


@pytest.mark.parametrize('dim,f32,n_sensors', GEM_CASES)
def test_gem_end_to_end_through_the_numpy_engine(dim, f32, n_sensors):
    case = planted_case(dim, 8, f32)
    gem_end_to_end(NumpyEngine(), case, n_sensors or case['s'])


def test_augment_placement_on_the_lattice_through_the_double():
    case = planted_case(3, 8)
    sens, lead = augment_picks(DesignEngine(), case)
    assert lead > 1e-3 and np.isin(sens, case['rows']).all()
    cells = set((sens % case['n_points']).tolist())
    assert cells & set(case['kept']) and not cells & set(case['gone'])
    pos = case['xyz'][sens % case['n_points']]
    d = np.linalg.norm(pos[:, None] - pos[None], axis=2) + 10.0 * np.eye(len(sens))
    assert d.min() >= case['d_min']
    # the picks hang on the flipped cells here too
    assert not np.array_equal(augment_picks(DesignEngine(), case, np.nextafter(case['d_min'], np.inf))[0], sens)
    assert not np.array_equal(augment_picks(DesignEngine(), case, np.nextafter(case['d_min'], 0.0))[0], sens)

"""GPU tests (-m gpu) of the three small kernels constrained placement rests on (csrc/qr_pivot.hip): qr_exclude_kernel and
mask_rows_kernel called directly, the within() test inside the candidate steps (qr_step_fused_kernel for r <= 128,
qr_cand_downdate_wide_kernel above), and GEM / augment_placement end to end -- against the literal NumPy expressions of
tests/test_exclude_host.py, on random grids and on the lattices whose d_min sphere passes through lattice points.  Every
assertion is exact: bits of nrm / of the basis, or the picks."""
import numpy as np
import pytest

from tests.test_design_host import DesignEngine
from tests.test_exclude_host import (GEM_CASES, QR_BATCH, augment_picks, check_planted, gem_end_to_end, in_step_picks,
                                     lattice_case, np_exclude, np_mask_rows, planted_case)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- qr_exclude -----------------------------------------------------------------------------------------------------------
def run_exclude(eng, nrm, row0, n_points, mask, xyz, picks, d_min, nq=None):
    """engine.qr_exclude through a hand-built state -> nrm afterwards"""
    t = eng.torch
    picks = np.asarray(picks, dtype=np.int64)
    st = dict(nrm=eng.to_device(np.array(nrm)), n=len(nrm), row0=row0,
              piv=eng.to_device(picks, dtype=t.int64) if len(picks) else None)
    eng.qr_exclude(st, mask=eng.to_device(mask.astype(np.uint8), dtype=t.uint8) if mask is not None else None,
                   xyz=eng.to_device(np.array(xyz)) if xyz is not None else None, n_points=n_points, j0=0,
                   nq=len(picks) if nq is None else nq, d_min=float(d_min))
    return np.asarray(eng.to_host(st['nrm']))


def norms_before(rng, n):
    nrm = rng.random(n) + 0.25
    nrm[rng.random(n) < 0.1] = -1.0                          # rows that left the race earlier
    nrm[rng.random(n) < 0.1] = 0.0                           # rows already in the span of the picks
    return nrm


def grid_case(dim, F, n_points, shard=False, picks='any', nq=QR_BATCH, mask=True, xyz=True, d_min='ring', seed=0):
    """Coordinates on a coarse grid (multiples of 1/20: many cells at equal distances, many exactly ON the sphere) and a d_min
    that is the distance NumPy gives between the first pick's cell and another cell (about 0.3)."""
    rng = np.random.default_rng(1000 * dim + 10 * F + seed)
    row0, n = (n_points + 13, n_points + 40) if shard else (0, F * n_points)
    pts = rng.integers(0, 21, (n_points, dim)) / 20.0
    hi = n_points if picks == 'feature 0' else F * n_points
    piv = rng.integers(0, hi, nq).astype(np.int64)
    if picks == 'none':
        piv[:] = -1
    elif nq > 2:
        piv[[1, nq - 1]] = -1                                # slots without a pick
    if nq and picks != 'none':
        d = np.linalg.norm(pts[piv[0] % n_points] - pts, axis=1)
        ring = float(d[np.argmin(np.abs(np.where(d > 0, d, 9.0) - 0.3))])
        assert np.any(d == ring)                             # a cell exactly at d_min: `<` keeps it
    else:
        ring = 0.3
    d_min = {'ring': ring, 'zero': 0.0, 'huge': 10.0}[d_min]
    return dict(nrm=norms_before(rng, n), row0=row0, n_points=n_points, mask=(rng.random(n) < 0.7) if mask else None,
                xyz=pts if xyz else None, picks=piv, d_min=d_min)


SHAPES = [(1, 67), (3, 1000)]                                # (F, n_points): neither a multiple of the 256-thread block
EXCLUDE_CASES = {f'{dim}d-F{F}-n{npt}': dict(dim=dim, F=F, n_points=npt)
                 for dim in (1, 2, 3) for F, npt in SHAPES}
EXCLUDE_CASES.update({f'{dim}d-n{npt}-shard-inside-a-feature': dict(dim=dim, F=3, n_points=npt, shard=True)
                      for dim in (1, 2, 3) for npt in (67, 1000)})
EXCLUDE_CASES.update({
    'picks-in-feature-0-rows-in-1-and-2': dict(dim=3, F=3, n_points=1000, shard=True, picks='feature 0'),
    'one-pick': dict(dim=3, F=3, n_points=1000, nq=1),
    'one-pick-2d-shard': dict(dim=2, F=3, n_points=67, nq=1, shard=True),
    'mask-only': dict(dim=3, F=3, n_points=1000, nq=0, xyz=False),
    'mask-only-xyz-given': dict(dim=2, F=3, n_points=67, nq=0),
    'xyz-only': dict(dim=3, F=3, n_points=1000, mask=False),
    'xyz-only-1d': dict(dim=1, F=3, n_points=67, mask=False, shard=True),
    'd_min-zero': dict(dim=3, F=3, n_points=1000, mask=False, d_min='zero'),
    'd_min-larger-than-the-domain': dict(dim=3, F=3, n_points=1000, mask=False, d_min='huge'),
    'no-pick-in-any-slot': dict(dim=2, F=3, n_points=1000, picks='none', d_min='huge'),
})


@pytest.mark.parametrize('name', sorted(EXCLUDE_CASES))
def test_qr_exclude_equals_the_literal_expression(eng, name):
    assert eng.qr_batch == QR_BATCH
    kw = dict(EXCLUDE_CASES[name])
    case = grid_case(kw.pop('dim'), kw.pop('F'), kw.pop('n_points'), **kw)
    want = np_exclude(**case)
    got = run_exclude(eng, **case)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(got[want != -1.0]), bits(case['nrm'][want != -1.0]))     # untouched entries keep their bits
    if name == 'd_min-zero':                                 # not even the pick's own cell goes
        np.testing.assert_array_equal(bits(got), bits(case['nrm']))
    if name == 'd_min-larger-than-the-domain':
        assert np.all(got == -1.0)
    if name == 'no-pick-in-any-slot':
        np.testing.assert_array_equal(bits(got), bits(np_exclude(case['nrm'], 0, 1000, case['mask'], None, [], 0.0)))
    if name == '3d-F3-n1000':                                # the pick's cell goes in EVERY feature
        cells = case['picks'][case['picks'] >= 0] % 1000
        assert np.all(got[(cells[:, None] + 1000 * np.arange(3)[None, :]).ravel()] == -1.0)


def test_qr_exclude_grid_stride(eng):
    """more rows than the 4096 x 256 threads of the launch: every thread takes a second row"""
    rng = np.random.default_rng(11)
    n = 4096 * 256 + 300
    xyz = rng.random((n, 3))
    piv = rng.integers(0, n, QR_BATCH)
    piv[3] = -1
    nrm = norms_before(rng, n)
    want = np_exclude(nrm, 0, n, None, xyz, piv, 0.2)
    assert 100 < np.sum((want == -1.0) & (nrm != -1.0)) and np.any(want[4096 * 256:] != nrm[4096 * 256:])
    np.testing.assert_array_equal(bits(run_exclude(eng, nrm, 0, n, None, xyz, piv, 0.2)), bits(want))


@pytest.mark.parametrize('shard', [False, True], ids=['whole', 'shard-inside-a-feature'])
@pytest.mark.parametrize('dim', [2, 3])
def test_qr_exclude_on_the_lattices(eng, dim, shard):
    """cells ON the d_min sphere: the kernel takes NumPy's decision for each of them (a fused sum of squares does not)"""
    case = lattice_case(dim)
    n_points, F = case['n_points'], 3
    row0, n = (n_points + 13, n_points + 40) if shard else (0, F * n_points)
    rng = np.random.default_rng(dim)
    nrm = norms_before(rng, n)
    picks = case['centres'] + (2 if shard else 1) * n_points  # the picks' feature is not (all of) the rows'
    want = np_exclude(nrm, row0, n_points, None, case['xyz'], picks, case['d_min'])
    got = run_exclude(eng, nrm, row0, n_points, None, case['xyz'], picks, case['d_min'])
    cell = (row0 + np.arange(n)) % n_points
    kept, gone = np.isin(cell, case['kept']), np.isin(cell, case['gone'])
    assert kept.any() and gone.any() and np.all(want[gone] == -1.0) and np.array_equal(want[kept], nrm[kept])
    print(f'{dim}-D lattice: rows on the sphere decided otherwise by a fused sum: kept {np.flatnonzero(kept & (got != want)).tolist()} '
          f'gone {np.flatnonzero(gone & (got != want)).tolist()}')
    np.testing.assert_array_equal(bits(got), bits(want))


def test_qr_exclude_refuses_what_it_cannot_do(eng):
    nrm, xyz = np.ones(100), np.random.default_rng(0).random((100, 3))
    with pytest.raises(ValueError):
        run_exclude(eng, nrm, 0, 100, None, xyz, np.arange(QR_BATCH + 1), 0.1)        # more picks than one call takes
    with pytest.raises(ValueError):
        run_exclude(eng, nrm, 0, 100, None, None, np.arange(3), 0.1)                  # picks without coordinates


# ---- mask_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', [0, 1, 2])
@pytest.mark.parametrize('n,r', [(1, 1), (257, 3), (1000, 129), (70001, 31)])        # the last: more elements than 8192 x 256 threads
@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
def test_mask_rows_equals_the_literal_expression(eng, dtype, n, r, pad):
    t = eng.torch
    rng = np.random.default_rng(n + r + pad)
    U = rng.standard_normal((n, r)).astype(dtype)
    U.ravel()[::5] = -0.0                                    # values whose bits tell them from the +0 of a masked row
    U.ravel()[::13] = np.inf
    mask = rng.random(n) < 0.5
    if n == 1:
        mask[:] = False
    buf = np.full((n, r + pad), -7.5, dtype=dtype)           # sentinels in the padding up to the leading dimension
    buf[:, :r] = U
    dev = eng.to_device(buf, dtype=t.float32 if dtype == np.float32 else t.float64)
    view = dev[:, :r]
    assert view.stride(0) == r + pad
    eng.mask_rows(view, eng.to_device(mask.astype(np.uint8), dtype=t.uint8))
    want = buf.copy()
    want[:, :r] = np_mask_rows(U, mask)
    got = np.asarray(eng.to_host(dev))
    assert got.dtype == dtype
    np.testing.assert_array_equal(bits(got), bits(want))     # kept rows and the padding bit for bit, masked rows +0


# ---- the within() test inside the candidate steps ---------------------------------------------------------------------------
@pytest.mark.parametrize('r', [8, 64, 128, 131])             # 4, 32 and 64 lanes per row of the fused step kernel; the wide kernel
@pytest.mark.parametrize('dim', [2, 3])
def test_in_step_exclusion_picks_the_oracles_rows(eng, dim, r):
    case = planted_case(dim, r)
    want = check_planted(case)
    got = in_step_picks(eng, eng.to_device(np.array(case['Ur'])), eng.to_device(np.array(case['xyz'])), case['n_points'],
                        case['d_min'], case['s'])
    print(f'{dim}-D r={r}: picks {got.tolist()} oracle {want.tolist()}')
    np.testing.assert_array_equal(got, want)


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,f32,n_sensors', GEM_CASES)
def test_gem_on_the_lattices_picks_the_oracles_rows(eng, dim, f32, n_sensors):
    case = planted_case(dim, 8, f32)
    check_planted(case)
    gem_end_to_end(eng, case, n_sensors or case['s'])


def test_augment_placement_on_the_lattice_picks_the_doubles_rows(eng):
    case = planted_case(3, 8)
    want, lead = augment_picks(DesignEngine(), case)
    assert lead > 1e-3
    got, _ = augment_picks(eng, case)
    print(f'augment_placement: picks {got.tolist()} double {want.tolist()}')
    np.testing.assert_array_equal(got, want)

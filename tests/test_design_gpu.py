"""The design sweep (csrc/design.hip) and SPR.augment_placement / placement_gain / optimal_placement('dopt' | 'aopt') on the
HIP engine: the score map entrywise against an np.longdouble restatement, the record, one block beyond 2^31 elements, and
the public methods end to end against the NumPy double of tests/test_design_host.py on its seeded cases.

Bar (derived, not measured).  With za = |B| |u|, da = |u|^T za, qa = za^T za, c = 4 (r + 4), eps = 2^-52:
    D:  c eps w da                                        A:  c eps (w qa / (1 + w d) + score w da / (1 + w d))
The rounding of two chained length-r dot products is below 3 r eps times these sums for any accumulation order; the
products with w, the sum 1 + w d and the division add a few eps of the terms themselves, which the 4 (r + 4) covers.
The best row of a record must be the oracle's whenever the oracle's lead exceeds the winner's bar plus the largest bar of
a row still in the race (asserted on the oracle, before the comparison); the runner-up VALUE is within that largest bar."""
import functools

import numpy as np
import pytest

from tests.test_design_host import CASES, DesignEngine, case_kwargs, draw_problem, fitted_spr, run_case

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -52
RANKS = [1, 5, 16, 33, 64, 100, 128]
SHAPES = [(1000, 3), (777, 2), (40, 1)]


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


def feature_of(n, row0, n_points, F):
    return np.minimum((row0 + np.arange(n)) // n_points, F - 1)


def oracle(U, B, w_rows, criterion):
    """-> (score, bar) per row, longdouble"""
    r = U.shape[1]
    Ul, Bl, w = U.astype(LD), B.astype(LD), w_rows.astype(LD)
    Z = Ul @ Bl
    d, q = (Z * Ul).sum(axis=1), (Z * Z).sum(axis=1)
    za = np.abs(Ul) @ np.abs(Bl)
    da, qa = (np.abs(Ul) * za).sum(axis=1), (za * za).sum(axis=1)
    c = LD(4 * (r + 4)) * LD(EPS)
    if criterion == 'D':
        return w * d, c * w * da
    score = w * q / (1 + w * d)
    return score, c * (w * qa / (1 + w * d) + score * w * da / (1 + w * d))


@functools.lru_cache(maxsize=None)
def problem(r, n_points, F, seed=0):
    """a seeded basis block, a symmetric positive definite B and distinct feature weights; shared, never modified"""
    rng = np.random.default_rng(1000 * r + n_points + seed)
    n = n_points * F
    U = rng.standard_normal((n, r)) / np.sqrt(r)
    A = rng.standard_normal((r, r))
    B = A @ A.T / r + 0.1 * np.eye(r)
    B = 0.5 * (B + B.T)
    wf = 0.5 + rng.uniform(size=F) * np.arange(1, F + 1)
    for a in (U, B, wf):
        a.setflags(write=False)
    return U, B, wf


def planted(B, scale=40.0):
    """a row that wins under both criteria: long (D: w d grows with its square) and along the top eigenvector of B (A:
    w q / (1 + w d) < q / d <= lambda_max, approached only there)"""
    return scale * np.linalg.eigh(B)[1][:, -1]


def check_record(rec, U, score, bar, alive_rows, row0, tag):
    """rec against the oracle over the rows `alive_rows` (local indices); U: the f64 values of the stored basis"""
    r = U.shape[1]
    if len(alive_rows) == 0:
        assert rec[0] == -np.inf and rec[1] == -1 and rec[2] == -np.inf and not np.any(rec[3:]), tag
        return
    s, b = score[alive_rows], bar[alive_rows]
    order = np.lexsort((alive_rows, -s.astype(np.float64)))
    i0 = order[0]
    if len(order) > 1:
        i1 = order[1]
        assert s[i0] == s[i1] or s[i0] - s[i1] > b[i0] + b.max(), (tag, 'the oracle lead is inside the bars: pick another seed')
        assert abs(LD(rec[2]) - s[i1]) <= b.max(), (tag, rec[2], s[i1])
    else:
        assert rec[2] == -np.inf, tag
    assert int(rec[1]) == row0 + alive_rows[i0], (tag, rec[1], row0 + alive_rows[i0])
    assert abs(LD(rec[0]) - s[i0]) <= b[i0], (tag, rec[0], s[i0])
    np.testing.assert_array_equal(rec[3:3 + r], U[alive_rows[i0]], err_msg=str(tag))     # bit-equal


def run_sweep(eng, Ud, U, B, wf, row0, n_points, F, criterion, alive=None, with_map=True):
    import torch
    n = U.shape[0]
    scores = eng.empty((n,)) if with_map else None
    alive_d = None if alive is None else eng.to_device(alive)
    rec = eng.design_sweep(Ud, row0, n_points, F, eng.to_device(np.array(B)), None if wf is None else eng.to_device(np.array(wf)),
                           alive_d,
                           criterion, scores=scores)
    torch.cuda.synchronize()
    return eng.to_host(rec).copy(), (None if scores is None else eng.to_host(scores).copy())


def check_sweep(eng, Ud, U, B, wf, row0, n_points, F, criterion, tag, alive=None):
    n = U.shape[0]
    w_rows = np.ones(n) if wf is None else wf[feature_of(n, row0, n_points, F)]
    score, bar = oracle(U, B, w_rows, criterion)
    rec, got = run_sweep(eng, Ud, U, B, wf, row0, n_points, F, criterion, alive)
    live = np.arange(n) if alive is None else np.flatnonzero(~(alive < 0))
    dead = np.setdiff1d(np.arange(n), live)
    assert np.all(got[dead] == -np.inf), tag
    err = np.abs(got[live].astype(LD) - score[live])
    ratio = float((err / bar[live]).max()) if len(live) else 0.0
    print('design', tag, criterion, 'worst error / bar', ratio)
    assert np.all(err <= bar[live]), (tag, ratio)
    check_record(rec, U, score, bar, live, row0, tag)
    rec2, _ = run_sweep(eng, Ud, U, B, wf, row0, n_points, F, criterion, alive, with_map=False)   # d_scores = NULL
    np.testing.assert_array_equal(rec2, rec)
    return rec, got


# ---- the score map and the record, full blocks ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('r', RANKS)
def test_score_map_and_record(eng, r, shape):
    n_points, F = shape
    U, B, wf = problem(r, n_points, F)
    Ud = eng.to_device(np.array(U))
    for criterion in ('D', 'A'):
        check_sweep(eng, Ud, U, B, wf, 0, n_points, F, criterion, (r, shape))
    check_sweep(eng, Ud, U, B, None, 0, n_points, F, 'A', (r, shape, 'no weights'))


@pytest.mark.parametrize('r', [5, 64, 100])
def test_block_that_starts_inside_a_feature(eng, r):
    U, B, wf = problem(r, 1000, 3)
    U = U[300:1800]
    Ud = eng.to_device(np.array(U))
    for criterion in ('D', 'A'):
        check_sweep(eng, Ud, U, B, wf, 300, 1000, 3, criterion, (r, 'row0 = 300'))


@pytest.mark.parametrize('r', [16, 33, 64])
def test_leading_dimension_and_unaligned_view(eng, r):
    U, B, wf = problem(r, 777, 2)
    n = U.shape[0]
    buf = np.zeros((n, r + 6))
    buf[:, 1:1 + r] = U
    wide = eng.to_device(buf)
    odd = wide[:, 1:1 + r]                                    # rows start 8 bytes off a 16-byte boundary: the scalar load path
    assert odd.stride(0) == r + 6 and odd.data_ptr() % 16 == 8
    check_sweep(eng, odd, U, B, wf, 0, 777, 2, 'A', (r, 'odd column'))
    buf2 = np.full((n, r + 6), 7.0)
    buf2[:, :r] = U
    even = eng.to_device(buf2)[:, :r]                         # ldu > r, 16-byte rows when r is even
    check_sweep(eng, even, U, B, wf, 0, 777, 2, 'D', (r, 'ldu > r'))


@pytest.mark.parametrize('r', [5, 64, 128])
def test_f32_stored_basis(eng, r):
    import torch
    U, B, wf = problem(r, 777, 2)
    U32 = U.astype(np.float32)
    Ud = eng.to_device(U32, dtype=torch.float32)
    for criterion in ('D', 'A'):
        check_sweep(eng, Ud, U32.astype(np.float64), B, wf, 0, 777, 2, criterion, (r, 'f32'))


# ---- the record: planted winners, dead rows, ties ------------------------------------------------------------------------
@pytest.mark.parametrize('r', [5, 33, 128])
@pytest.mark.parametrize('where', ['first', 'last of a partial panel', 'last'])
def test_planted_winner(eng, r, where):
    U, B, wf = problem(r, 777, 2)                             # 777 = 12 x 64 + 9: every feature ends in a partial panel
    U = U.copy()
    row = {'first': 0, 'last of a partial panel': 776, 'last': 1553}[where]
    U[row] = planted(B)
    Ud = eng.to_device(np.array(U))
    for criterion in ('D', 'A'):
        rec, _ = check_sweep(eng, Ud, U, B, None, 0, 777, 2, criterion, (r, where))
        assert int(rec[1]) == row


@pytest.mark.parametrize('r', [16, 100])
def test_dead_rows_and_dead_panels(eng, r):
    U, B, wf = problem(r, 1000, 3)
    U = U.copy()
    U[130] = planted(B)                                       # the row that would win lies in a dead panel
    n = U.shape[0]
    rng = np.random.default_rng(r)
    alive = np.zeros(n)
    alive[64:256] = -1.0                                      # three whole panels
    alive[1000:1064] = -3.5                                   # the first panel of feature 1
    alive[rng.choice(n, 200, replace=False)] = -1.0
    alive[5] = 2.0                                            # positive and zero entries are in the race
    Ud = eng.to_device(np.array(U))
    for criterion in ('D', 'A'):
        rec, got = check_sweep(eng, Ud, U, B, wf, 0, 1000, 3, criterion, (r, 'dead rows'), alive=alive)
        assert int(rec[1]) != 130 and got[130] == -np.inf
    # one row left; nobody left
    one = np.full(n, -1.0)
    one[2999] = 0.0
    rec, _ = check_sweep(eng, Ud, U, B, wf, 0, 1000, 3, 'D', (r, 'one row'), alive=one)
    assert int(rec[1]) == 2999 and rec[2] == -np.inf
    rec, got = check_sweep(eng, Ud, U, B, wf, 0, 1000, 3, 'A', (r, 'all dead'), alive=np.full(n, -1.0))
    assert int(rec[1]) == -1 and rec[0] == -np.inf and np.all(got == -np.inf)


@pytest.mark.parametrize('r', [5, 64])
def test_tie_the_lower_row_wins(eng, r):
    U, B, wf = problem(r, 777, 2)
    U = U.copy()
    U[70] = planted(B)
    U[500] = U[70]                                            # same feature, same weight: the same score bit for bit
    U[775] = U[70]
    Ud = eng.to_device(np.array(U))
    for criterion in ('D', 'A'):
        rec, got = check_sweep(eng, Ud, U, B, wf, 0, 777, 2, criterion, (r, 'tie'))
        assert int(rec[1]) == 70 and rec[2] == rec[0] and got[70] == got[500] == got[775]
    alive = np.zeros(U.shape[0])
    alive[70] = -1.0                                          # the duplicate may be taken once the first is out
    rec, _ = check_sweep(eng, Ud, U, B, wf, 0, 777, 2, 'D', (r, 'tie, first out'), alive=alive)
    assert int(rec[1]) == 500


def test_nan_never_wins(eng):
    U, B, wf = problem(16, 777, 2)
    U = U.copy()
    U[3, 2] = np.nan
    Ud = eng.to_device(np.array(U))
    rec, got = run_sweep(eng, Ud, U, B, wf, 0, 777, 2, 'D')
    assert np.isnan(got[3]) and int(rec[1]) != 3 and np.isfinite(rec[0]) and np.isfinite(rec[2])
    assert int(rec[1]) == int(np.nanargmax(got))


# ---- addressing beyond 32 bits --------------------------------------------------------------------------------------------
def test_block_with_more_than_2_31_elements(eng):
    """2^25 + 77 rows of r = 64: element offsets pass 2^31 (17 GB of basis).  The reference is the same formula evaluated
    with torch on the device in chunks, under the same bar."""
    import torch
    r, n = 64, (1 << 25) + 77
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    Ud = torch.randn((n, r), generator=g, device=dev, dtype=torch.float64) / 8.0
    _, B, _ = problem(r, 40, 1)
    Ud[n - 1] = eng.to_device(planted(B, 30.0))               # the winner is the last row
    wf = np.array([1.7])
    Bd = eng.to_device(np.array(B))
    scores = eng.empty((n,))
    rec = eng.to_host(eng.design_sweep(Ud, 0, n, 1, Bd, eng.to_device(wf), None, 'A', scores=scores)).copy()
    c = 4 * (r + 4) * EPS
    worst = 0.0
    for i0 in range(0, n, 1 << 22):
        u = Ud[i0:i0 + (1 << 22)]
        z = u @ Bd
        d, q = (z * u).sum(1), (z * z).sum(1)
        za = u.abs() @ Bd.abs()
        da, qa = (u.abs() * za).sum(1), (za * za).sum(1)
        ref = 1.7 * q / (1 + 1.7 * d)
        bar = c * (1.7 * qa / (1 + 1.7 * d) + ref * 1.7 * da / (1 + 1.7 * d))
        ratio = ((scores[i0:i0 + (1 << 22)] - ref).abs() / bar).max().item()
        worst = max(worst, ratio)
    print('design 2^31 worst error / bar', worst)
    assert worst <= 1.0
    assert int(rec[1]) == n - 1 and rec[0] == scores[n - 1].item()
    np.testing.assert_array_equal(rec[3:], eng.to_host(Ud[n - 1]))
    top2 = torch.topk(scores, 2).values
    assert rec[0] == top2[0].item() and rec[2] == top2[1].item()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def double_run(name, criterion):
    """the NumPy double on a seeded case -> (basis, Ar, qr sensors + additions, design_info_)"""
    case = CASES[name]
    spr = fitted_spr(case)
    sens, gap, info = run_case(spr, case, criterion)
    return np.array(spr.Ur), np.array(spr.Ar), sens, gap, info


def gpu_spr(eng, name, criterion):
    from openmeasure_amd.sparse_sensing import SPR
    case = CASES[name]
    X, xyz = draw_problem(case['seed'], case['n_points'], case['F'], case['m'], case['r'])
    Ur, Ar, sens, gap, info = double_run(name, criterion)
    spr = SPR(X, case['F'], xyz, engine=eng)
    spr.fit(basis=(Ur, Ar))                                  # the double's basis: the comparison is of the placement alone
    return spr, case, sens, info


@pytest.mark.parametrize('criterion', ['D', 'A'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_augment_placement_picks_the_doubles_sensors(eng, name, criterion):
    spr, case, sens, info = gpu_spr(eng, name, criterion)
    Ur_before = spr.Ur.copy()
    got, gap, ginfo = run_case(spr, case, criterion)
    np.testing.assert_array_equal(got, sens)
    for key in ('logdet', 'trace_inv'):
        np.testing.assert_allclose(ginfo[key], info[key], rtol=1e-10)
    # gain is the kernel's winning score: the kernel and the double each carry 4 (r + 4) eps da / d of it (the bar of the
    # module docstring) with da / d <= sqrt(r) cond(M), and cond(M) <= 60 on these cases (design_info_['cond']):
    # 4 (33 + 4) 2.2e-16 sqrt(33) 60 = 1.1e-11 per side -- inside the 1e-10 of the trajectories
    assert max(info['cond']) <= 60
    np.testing.assert_allclose(ginfo['gain'], info['gain'], rtol=1e-10)
    assert spr.pivot_sweeps_ == case['extra'] and gap[case['r']:].min() >= 1e-6 / 2
    again, _, ainfo = run_case(spr, case, criterion)             # two runs: bit-identical
    np.testing.assert_array_equal(again, got)
    for key in ('logdet', 'trace_inv', 'gain', 'cov'):
        np.testing.assert_array_equal(ainfo[key], ginfo[key])
    np.testing.assert_array_equal(np.asarray(eng.to_host(spr._d['Ur'])), Ur_before)   # the basis is not modified


@pytest.mark.parametrize('calc', ['dopt', 'aopt'])
@pytest.mark.parametrize('name', ['r5', 'r16', 'r33-dmin'])
def test_optimal_placement_dopt_aopt(eng, name, calc):
    spr, case, sens, info = gpu_spr(eng, name, calc[0].upper())
    r, n = case['r'], case['n_points'] * case['F']
    C = spr.optimal_placement(calc, n_sensors=r + case['extra'], d_min=case.get('d_min', 0.))
    np.testing.assert_array_equal(spr.sensors_, sens)
    assert C.shape == (r + case['extra'], n)
    with pytest.raises(ValueError):
        spr.optimal_placement(calc, n_sensors=r - 1)
    # train, predict and reconstruct accept the oversampled placement
    spr.train(C)
    fid = spr.sensors_ // spr.n_points
    X, _ = draw_problem(case['seed'], case['n_points'], case['F'], case['m'], case['r'])
    y = np.stack([X[spr.sensors_, 0], np.full(len(fid), 0.1), fid.astype(float)], axis=1)
    Ar, As = spr.predict(y)
    assert Ar.shape == (1, r) and np.all(np.isfinite(Ar)) and np.all(np.isfinite(As))
    field = spr.reconstruct(Ar)
    assert field.shape == (n, 1) and np.all(np.isfinite(field))
    cov = spr.coefficient_covariance(y)[0]
    w = (spr._scl_f[fid] / 0.1) ** 2
    np.testing.assert_allclose(np.trace(cov), np.trace(np.linalg.inv((spr.Theta * w[:, None]).T @ spr.Theta)), rtol=1e-8)


@pytest.mark.parametrize('criterion', ['D', 'A'])
def test_placement_gain_is_the_kernel_map(eng, criterion):
    spr, case, sens, info = gpu_spr(eng, 'r16-noise', criterion)
    noise = case_kwargs(case)['noise']
    spr.optimal_placement('qr')
    gain = spr.placement_gain(criterion, noise=noise)
    U = np.asarray(spr.Ur)
    n, r = U.shape
    wf = (spr._scl_f / noise) ** 2
    w_rows = wf[feature_of(n, 0, case['n_points'], case['F'])]
    Th = U[spr.sensors_]
    M = (Th * w_rows[spr.sensors_][:, None]).T @ Th
    score, bar = oracle(U, np.linalg.inv(M), w_rows, criterion)
    # B is formed by the driver from its own factorisation: compare at the bar widened by cond(M) eps of the inverse
    slack = LD(np.linalg.cond(M) * 16 * r * EPS)
    assert np.all(np.abs(gain.astype(LD) - score) <= bar + slack * np.abs(score))
    # ... and bit for bit the map of one sweep with the driver's own inverse
    from openmeasure_amd._design import _inverse
    Md = spr._design_matrix(eng, spr._d['Ur'], spr.sensors_, wf, np.zeros(r))
    direct = eng.empty((n,))
    eng.design_sweep(spr._d['Ur'], 0, case['n_points'], case['F'], eng.to_device(_inverse(Md)[0]), eng.to_device(wf), None,
                     criterion, scores=direct)
    np.testing.assert_array_equal(eng.to_host(direct), gain)
    dev = spr.placement_gain(criterion, noise=noise, to_host=False)
    np.testing.assert_array_equal(eng.to_host(dev), gain)       # two runs agree bit for bit
    assert spr.placement_gain(criterion, sensors=spr.sensors_[:3], ridge=0.5).shape == (n,)


def test_the_double_and_the_engine_share_an_interface():
    import inspect
    from openmeasure_amd.engine import HipEngine
    assert (inspect.signature(HipEngine.design_sweep).parameters.keys()
            == inspect.signature(DesignEngine.design_sweep).parameters.keys())

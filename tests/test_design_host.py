"""Oversampled sensor placement (openmeasure_amd/_design.py) on the CPU: the host driver over a NumPy double of the design
sweep (csrc/design.hip) -- picks against brute force that never uses the score formulas, design_info_ against direct
values and against coefficient_covariance, start= in its three forms, exclusions and ties, 'dopt' / 'aopt' of
optimal_placement, exhausted candidates, a world-size-2 run over gloo, and the smallest relative lead of the seeded cases
the GPU tests reuse (tests/test_design_gpu.py imports DesignEngine, CASES and the builders from here)."""
import os
import sys

import numpy as np
import pytest
import torch

from openmeasure_amd.sparse_sensing import SPR
from openmeasure_amd.rom import OneHotRows
from tests.numpy_engine import NumpyEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DesignEngine(NumpyEngine):
    """NumpyEngine + the design sweep: what the kernel computes, not how."""

    def design_sweep(self, Ur, row0, n_points, n_features, B, wfeat=None, alive=None, criterion='D', scores=None):
        U = self._w(Ur)
        n, r = U.shape
        w = np.ones(n) if wfeat is None else wfeat.numpy()[self._feat(n, row0, n_points, n_features)]
        Z = U @ B.numpy()
        d, q = (Z * U).sum(axis=1), (Z * Z).sum(axis=1)
        sc = w * d if criterion == 'D' else w * q / (1.0 + w * d)
        if alive is not None:
            sc = np.where(alive.numpy() < 0, -np.inf, sc)
        if scores is not None:
            scores.numpy()[:] = sc
        cand = np.where(np.isnan(sc), -np.inf, sc)
        rec = np.zeros(r + 3)
        rec[:3] = -np.inf, -1.0, -np.inf
        if np.any(cand > -np.inf):
            i = int(np.argmax(cand))                          # first index on ties
            rec[0], rec[1], rec[3:] = cand[i], row0 + i, U[i]
            rec[2] = np.max(np.delete(cand, i)) if n > 1 else -np.inf
        return torch.from_numpy(rec)


# ---- seeded problems: low rank plus noise, feature-major rows ---------------------------------------------------------
def draw_problem(seed, n_points, F, m, r):
    rng = np.random.default_rng(seed)
    n, k = n_points * F, r + 2
    X = (rng.standard_normal((n, k)) * 2.0 ** (-0.5 * np.arange(k))) @ rng.standard_normal((k, m))
    X += 0.02 * rng.standard_normal((n, m))
    for f in range(F):
        X[f * n_points:(f + 1) * n_points] = (1.0 + f) * X[f * n_points:(f + 1) * n_points] + 3.0 * f
    xyz = rng.uniform(0.0, 1.0, (n_points, 2))
    return X, xyz


def fitted_spr(case, engine=None, shard=None, rows=slice(None)):
    X, xyz = draw_problem(case['seed'], case['n_points'], case['F'], case['m'], case['r'])
    spr = SPR(np.ascontiguousarray(X[rows]), case['F'], xyz, engine=engine or DesignEngine(), shard=shard)
    spr.fit(select_modes='number', n_modes=case['r'])
    return spr


def case_kwargs(case):
    """noise / mask / d_min of a case -> keyword arguments of augment_placement"""
    kw = {}
    n = case['n_points'] * case['F']
    rng = np.random.default_rng(case['seed'] + 1000)
    if case.get('noise'):
        kw['noise'] = rng.uniform(0.05, 0.5, case['F'])
    if case.get('mask'):
        kw['mask'] = rng.uniform(size=n) < 0.7
    if case.get('d_min'):
        kw['d_min'] = case['d_min']
    return kw


TINY = [dict(seed=s, n_points=20, F=3, m=10, r=r, extra=4, noise=nz) for s, r, nz in
        ((1, 3, False), (2, 4, True), (3, 5, False), (4, 6, True))]
# the cases the GPU tests reuse (sensors identical to this double's): r below, at and between the tile widths
CASES = {
    'r5': dict(seed=11, n_points=300, F=3, m=12, r=5, extra=6),
    'r5-noise-mask-dmin': dict(seed=12, n_points=300, F=3, m=12, r=5, extra=6, noise=True, mask=True, d_min=0.03),
    'r16': dict(seed=13, n_points=500, F=2, m=24, r=16, extra=6),
    'r16-noise': dict(seed=14, n_points=500, F=2, m=24, r=16, extra=6, noise=True),
    'r33-dmin': dict(seed=15, n_points=400, F=2, m=40, r=33, extra=4, d_min=0.02),
}


def info_matrix(U, rows, w_rows, ridge=0.0):
    Th = U[rows]
    return np.diag(np.full(U.shape[1], ridge)) + (Th * w_rows[:, None]).T @ Th


def row_weights(spr, rows, noise):
    f = np.asarray(rows) // spr.n_points
    return np.ones(len(rows)) if noise is None else (spr._scl_f[f] / np.asarray(noise)[f]) ** 2


# ---- against brute force ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('criterion', ['D', 'A'])
@pytest.mark.parametrize('case', TINY, ids=lambda c: f"r{c['r']}")
def test_picks_equal_brute_force(case, criterion):
    spr = fitted_spr(case)
    r, n = case['r'], case['n_points'] * case['F']
    noise = case_kwargs(case).get('noise')
    spr.optimal_placement('qr')
    start = spr.sensors_.copy()
    spr.augment_placement(r + case['extra'], criterion, noise=noise)
    U = np.asarray(spr.Ur)
    sens = spr.sensors_
    assert sens.shape == (r + case['extra'],) and np.array_equal(sens[:r], start)
    assert spr.pivot_sweeps_ == case['extra'] and np.all(spr.pivot_gap_[:r] == 0)
    wall = row_weights(spr, np.arange(n), noise)
    info = spr.design_info_
    for j in range(r, len(sens)):
        M = info_matrix(U, sens[:j], wall[sens[:j]])
        if criterion == 'D':
            val = np.array([np.linalg.slogdet(M + wall[i] * np.outer(U[i], U[i]))[1] for i in range(n)])
        else:
            val = -np.array([np.trace(np.linalg.inv(M + wall[i] * np.outer(U[i], U[i]))) for i in range(n)])
        val[sens[:j]] = -np.inf
        assert sens[j] == int(np.argmax(val)), (j, sens[j], int(np.argmax(val)))
        np.testing.assert_allclose(info['logdet'][j - r], np.linalg.slogdet(M)[1], rtol=1e-10)
        np.testing.assert_allclose(info['trace_inv'][j - r], np.trace(np.linalg.inv(M)), rtol=1e-10)
    M = info_matrix(U, sens, wall[sens])
    np.testing.assert_allclose(info['logdet'][-1], np.linalg.slogdet(M)[1], rtol=1e-10)
    np.testing.assert_allclose(info['trace_inv'][-1], np.trace(np.linalg.inv(M)), rtol=1e-10)
    assert len(info['logdet']) == len(info['trace_inv']) == case['extra'] + 1 and len(info['gain']) == case['extra']
    assert info['criterion'] == criterion and info['cond'][1] <= info['cond'][0] * (1 + 1e-9)
    if criterion == 'D':
        np.testing.assert_allclose(np.diff(info['logdet']), np.log1p(info['gain']), rtol=1e-8)
    else:
        np.testing.assert_allclose(-np.diff(info['trace_inv']), info['gain'], rtol=1e-8)


def test_trace_and_cov_equal_coefficient_covariance():
    case = TINY[3]
    spr = fitted_spr(case)
    noise = case_kwargs(case)['noise']
    spr.optimal_placement('qr')
    C = spr.augment_placement(case['r'] + 5, 'A', noise=noise)
    spr.train(C)
    fid = spr.sensors_ // spr.n_points
    y = np.stack([np.zeros(len(fid)), noise[fid], fid.astype(float)], axis=1)
    cov = spr.coefficient_covariance(y)[0]
    np.testing.assert_allclose(np.trace(cov), spr.design_info_['trace_inv'][-1], rtol=1e-9)
    np.testing.assert_allclose(spr.design_info_['cov'], cov, rtol=1e-9, atol=1e-9 * np.abs(cov).max())
    Ar, _ = spr.predict(y)                                    # the oversampled placement is a valid training input
    assert Ar.shape == (1, case['r'])


# ---- start= -----------------------------------------------------------------------------------------------------------
def test_start_in_its_three_forms_and_the_default():
    case = TINY[2]
    spr = fitted_spr(case)
    r, n = case['r'], case['n_points'] * case['F']
    spr.optimal_placement('qr')
    start = spr.sensors_.copy()
    want = np.argmax(np.asarray(spr.augment_placement(r + 3)), axis=1)
    dense = np.zeros((r, n))
    dense[np.arange(r), start] = 1.0
    for form in (start, start.astype(np.int32), dense, OneHotRows(start, n)):
        C = spr.augment_placement(r + 3, start=form)
        assert C.shape == (r + 3, n)
        np.testing.assert_array_equal(spr.sensors_, want)
        np.testing.assert_array_equal(np.argmax(np.asarray(C), axis=1), want)
    # n_sensors is the total: equal returns the start with zero sweeps, smaller is refused
    C = spr.augment_placement(r, start=start)
    assert spr.pivot_sweeps_ == 0 and np.array_equal(spr.sensors_, start) and C.shape == (r, n)
    with pytest.raises(ValueError, match='TOTAL'):
        spr.augment_placement(r - 1, start=start)
    with pytest.raises(IndexError):
        spr.augment_placement(r + 1, start=np.array([0, n]))
    with pytest.raises(ValueError):
        spr.augment_placement(r + 1, start=np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match='criterion'):
        spr.augment_placement(r + 1, 'E', start=start)
    for bad in (np.ones(2), np.array([1.0, 0.0, np.nan]), np.array([1.0, -1.0, 1.0]), np.array([1.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match='noise'):
            spr.augment_placement(r + 1, start=start, noise=bad)


def test_no_earlier_placement_is_an_attribute_error():
    spr = fitted_spr(TINY[0])
    assert hasattr(spr, 'augment_placement') and hasattr(spr, 'placement_gain')
    with pytest.raises(AttributeError, match='sensors_'):
        spr.augment_placement(5)
    with pytest.raises(AttributeError, match='sensors_'):
        spr.placement_gain()


def test_gem_start_needs_a_ridge():
    case = TINY[3]
    spr = fitted_spr(case)
    r = case['r']
    spr.optimal_placement('gem', n_sensors=r - 2)
    gem = spr.sensors_.copy()
    with pytest.raises(ValueError, match='ridge'):
        spr.augment_placement(r + 2)
    assert np.array_equal(spr.sensors_, gem)                  # the refusal left the placement alone
    C = spr.augment_placement(r + 2, ridge=1e-3)
    assert C.shape[0] == r + 2 and np.array_equal(spr.sensors_[:r - 2], gem) and len(set(spr.sensors_)) == r + 2
    U = np.asarray(spr.Ur)
    M = info_matrix(U, spr.sensors_, np.ones(r + 2), 1e-3)
    np.testing.assert_allclose(spr.design_info_['trace_inv'][-1], np.trace(np.linalg.inv(M)), rtol=1e-9)
    # a ridge per mode, and an empty start
    spr.augment_placement(3, 'A', start=np.zeros(0, dtype=np.int64), ridge=np.full(r, 0.5))
    assert len(set(spr.sensors_)) == 3
    with pytest.raises(ValueError, match='ridge'):
        spr.augment_placement(r + 2, start=gem, ridge=-1.0)


# ---- exclusions and ties ----------------------------------------------------------------------------------------------
def test_mask_dmin_and_no_repeats():
    case = dict(seed=21, n_points=40, F=2, m=10, r=4)
    spr = fitted_spr(case)
    n = 80
    rng = np.random.default_rng(5)
    mask = rng.uniform(size=n) < 0.6
    xyz = np.asarray(spr.xyz)
    d_min = 0.1
    far = next(j for j in range(1, 40) if np.linalg.norm(xyz[0] - xyz[j]) >= d_min)
    start = np.array([0, 40 + far])                           # cell 0 of feature 0, a cell at least d_min away of feature 1
    C = spr.augment_placement(8, 'A', start=start, mask=mask, d_min=d_min, ridge=1e-2)
    sens = spr.sensors_
    assert C.shape[0] == 8 and len(set(sens.tolist())) == 8
    assert np.all(mask[sens[2:]])
    pos = xyz[sens % spr.n_points]
    dist = np.linalg.norm(pos[:, None] - pos[None], axis=2) + 10.0 * np.eye(8)
    assert dist.min() >= d_min
    # the same call without the exclusions picks something else: they did act
    spr.augment_placement(8, 'A', start=start, ridge=1e-2)
    assert not np.array_equal(spr.sensors_, sens)
    with pytest.raises(IndexError):
        spr.augment_placement(8, start=start, mask=mask[:-1], ridge=1e-2)


def test_duplicate_rows_the_lower_index_wins():
    case = TINY[1]
    spr = fitted_spr(case)
    spr.optimal_placement('qr')
    start = spr.sensors_.copy()
    gain = spr.placement_gain('D')
    gain[start] = -np.inf
    win = int(np.argmax(gain))
    dup = next(i for i in range(win + 1, len(gain)) if i not in start)
    U = np.array(spr.Ur)
    U[dup] = U[win]
    spr.Ur = U
    spr.augment_placement(len(start) + 2, 'D', start=start)
    assert spr.sensors_[len(start)] == win and spr.pivot_gap_[len(start)] == 0.0
    assert np.array_equal(np.asarray(spr.Ur), U)              # the basis is not modified
    assert spr.sensors_[len(start) + 1] != win                # no row appears twice
    # the duplicate stays in the race: it is taken as soon as the mask leaves nobody else
    only = np.zeros(len(gain), dtype=bool)
    only[dup] = True
    spr.augment_placement(len(start) + 2, 'D', start=np.append(start, win), mask=only)
    assert spr.sensors_[-1] == dup


def test_exhausted_candidates():
    case = TINY[0]
    spr = fitted_spr(case)
    spr.optimal_placement('qr')
    n = case['n_points'] * case['F']
    mask = np.zeros(n, dtype=bool)
    mask[spr.sensors_] = True
    free = [i for i in range(n) if i not in spr.sensors_][:2]
    mask[free] = True
    with pytest.raises(RuntimeError, match='no admissible row'):
        spr.augment_placement(case['r'] + 3, start=spr.sensors_.copy(), mask=mask)


# ---- optimal_placement('dopt' | 'aopt') --------------------------------------------------------------------------------
@pytest.mark.parametrize('calc', ['dopt', 'aopt'])
def test_dopt_aopt_start_from_the_qr_sensors(calc):
    case = TINY[2]
    spr = fitted_spr(case)
    r = case['r']
    C0 = np.asarray(spr.optimal_placement('qr'))
    qr, gap = spr.sensors_.copy(), spr.pivot_gap_.copy()
    C = spr.optimal_placement(calc, n_sensors=r + 4)
    assert C.shape[0] == r + 4 and np.array_equal(spr.sensors_[:r], qr)
    assert spr.design_info_['criterion'] == calc[0].upper()
    with pytest.raises(ValueError, match='smaller than the r'):
        spr.optimal_placement(calc, n_sensors=r - 1)
    C1 = np.asarray(spr.optimal_placement('qr'))
    np.testing.assert_array_equal(C0, C1)
    np.testing.assert_array_equal(spr.sensors_, qr)
    np.testing.assert_array_equal(spr.pivot_gap_, gap)
    # the same additions as augment_placement on the 'qr' placement
    want = spr.sensors_.copy()
    spr.augment_placement(r + 4, calc[0].upper())
    got = spr.sensors_.copy()
    spr.optimal_placement(calc, n_sensors=r + 4)
    np.testing.assert_array_equal(spr.sensors_, got)
    assert np.array_equal(got[:r], want)


def test_placement_gain_is_the_score_map():
    case = TINY[1]
    spr = fitted_spr(case)
    noise = case_kwargs(case)['noise']
    spr.optimal_placement('qr')
    U, sens = np.asarray(spr.Ur), spr.sensors_
    n = U.shape[0]
    wall = row_weights(spr, np.arange(n), noise)
    Minv = np.linalg.inv(info_matrix(U, sens, wall[sens]))
    d = np.einsum('ij,jk,ik->i', U, Minv, U)
    q = np.einsum('ij,jk,ik->i', U, Minv @ Minv, U)
    np.testing.assert_allclose(spr.placement_gain('D', noise=noise), wall * d, rtol=1e-9)
    np.testing.assert_allclose(spr.placement_gain('A', noise=noise), wall * q / (1 + wall * d), rtol=1e-9)
    assert spr.placement_gain('D', sensors=sens[:2], ridge=0.1).shape == (n,)


def test_rank_cap_is_refused_before_device_work():
    case = dict(seed=31, n_points=70, F=2, m=135, r=129)
    spr = fitted_spr(case)
    for call in (lambda: spr.augment_placement(140, start=np.arange(129)), lambda: spr.optimal_placement('dopt', n_sensors=140),
                 lambda: spr.placement_gain(sensors=np.arange(129))):
        with pytest.raises(NotImplementedError, match='128'):
            call()


# ---- the seeded cases the GPU tests reuse ------------------------------------------------------------------------------
def run_case(spr, case, criterion):
    spr.optimal_placement('qr')
    spr.augment_placement(case['r'] + case['extra'], criterion, **case_kwargs(case))
    return spr.sensors_.copy(), spr.pivot_gap_.copy(), spr.design_info_


@pytest.mark.parametrize('criterion', ['D', 'A'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_smallest_lead_of_the_shared_cases(name, criterion):
    case = CASES[name]
    sens, gap, info = run_case(fitted_spr(case), case, criterion)
    assert len(set(sens.tolist())) == case['r'] + case['extra']
    lead = gap[case['r']:].min()
    print(f'{name} {criterion}: smallest relative lead {lead:.3e}')
    assert lead >= 1e-6


# ---- world = 2 over gloo -----------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from openmeasure_amd.sparse_sensing import RowShard
        from tests.test_design_host import CASES, DesignEngine, fitted_spr, run_case
        out = {}
        for name in ('r5', 'r5-noise-mask-dmin'):
            case = CASES[name]
            n = case['n_points'] * case['F']
            cut = case['n_points'] + 77                           # the block boundary cuts through feature 1
            row0, n_loc = (0, cut) if rank == 0 else (cut, n - cut)
            spr = fitted_spr(case, DesignEngine(), RowShard(row0, n), slice(row0, row0 + n_loc))
            kw = case_kwargs(case)
            if 'mask' in kw:
                kw['mask'] = kw['mask'][row0:row0 + n_loc]
            for crit in ('D', 'A'):
                spr.optimal_placement('qr')
                spr.augment_placement(case['r'] + case['extra'], crit, **kw)
                out[f'{name}/{crit}'] = spr.sensors_.copy()
                out[f'{name}/{crit}/trace'] = spr.design_info_['trace_inv']
            with pytest.raises(NotImplementedError):
                spr.placement_gain()
        np.savez(os.path.join(out_dir, f'rank{rank}.npz'), **out)
    finally:
        dist.destroy_process_group()


def test_sharded_over_gloo_picks_the_same_sensors(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_dist_gloo import _free_port
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    outs = [np.load(tmp_path / f'rank{r}.npz') for r in range(2)]
    for name in ('r5', 'r5-noise-mask-dmin'):
        case = CASES[name]
        for crit in ('D', 'A'):
            sens, _, info = run_case(fitted_spr(case), case, crit)
            for o in outs:
                np.testing.assert_array_equal(o[f'{name}/{crit}'], sens)
                np.testing.assert_allclose(o[f'{name}/{crit}/trace'], info['trace_inv'], rtol=1e-8)

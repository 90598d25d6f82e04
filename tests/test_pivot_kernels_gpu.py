"""GPU tests (-m gpu) of the core of csrc/qr_pivot.hip at the level of its outputs: the squared row norms after
spr_qr_init_* / spr_qr_init_norms_* / spr_qr_refresh_*, the bound tau, the record, the certification flags, the gaps and
the directions of spr_qr_step_f64 / spr_qr_steps_f64 -- against the long-double references and the candidate model of
tests/test_pivot_kernels_host.py, on the cases built there (which file also shows, on the CPU, that every case has the
property it is used for).  The id of a sweep case names the kernel launch_refresh selects for it (direct-NG*, mfma-MTR*-LM*,
wide-NG*-vec/scalar), the id of a step case the step kernels (fused-LPR*-orth-NJ*, three-launch).  Columns outside a view
hold NaN: one element read past a row poisons the result.

Exact assertions: everything the model determines from the device's OWN norms -- tau, the record (value, row, runner-up, the
bits of the stored row), pivots, flags -- and the +-1 bases of group 3, whose norms are exact in any summation order.
Toleranced assertions use the bars derived in the host file's docstring; each prints its worst error / bar ratio and
test_zz_worst_ratio_overall asserts the maximum.  The bar of the directions rests on a measurement: the float64 NumPy double
of the step (NumpyEngine.qr_step) against the long-double Gram-Schmidt over the step cases gave, worst over the case list,
    |q - ref|_inf 2.05e-16      | |q| - 1 | 2.04e-16      |Q[:step] q|_inf 3.08e-16
(tests/test_pivot_kernels_host.py::test_twin_worst_values prints them); a device direction may err 8 times that plus r u.

Two pivoting states that are stepped alternately live on two engines: an engine keeps ONE 'qr' workspace (candidates, block
lists), so qr_begin for a second state overwrites the first state's candidates.  The product never steps two states of one
engine alternately (GEM's ridge phase opens its second state after the last step of the first)."""
import ctypes

import numpy as np
import pytest

from openmeasure_amd._placement import pivot_loop
from tests.test_pivot_kernels_host import (
    ALL_R, EXACT_N, EXACT_R, EXACT_SPOTS, GAP_BAR, LD, N_STRIDE, N_TABLE, PLANT_R, PLANT_R_POOLS, QR_BATCH, ROW0S, SHARD_R,
    SHARD_SPLITS, STEP_CALLS, STEP_ROW0, U_RND, apply_bar, basis, candidate_model, check_planted, device_cap, direction_errors,
    exact_basis, exact_residuals, greedy_pivots_ld, init_bar, layout_buffer, model_batch, model_record, orthonormal_rows,
    planted_basis, planted_norms, record_is_decided, ref_apply, ref_init, ref_step, refresh_picks, shard_basis, shard_steps,
    step_basis, step_count, step_family, sweep_cases, sweep_grid, sweep_id, tau_bounds, twin_direction_errors, twin_worst, widen)

pytestmark = pytest.mark.gpu

WORST = {}                                        # tag -> worst error / bar


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    e = HipEngine()
    assert e.qr_batch == QR_BATCH
    return e


@pytest.fixture(scope='module')
def eng2():
    from openmeasure_amd.engine import HipEngine
    return HipEngine()


@pytest.fixture(scope='module')
def cap(eng):
    cus = ctypes.c_int(0)
    assert eng.lib.spr_device_cus(ctypes.byref(cus)) == 0 and cus.value >= 3
    return device_cap(cus.value)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def host(eng, t):
    return np.array(eng.to_host(t))


def note(tag, ratio):
    ratio = float(ratio)
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    return ratio


def upload(eng, U, layout):
    """the basis as a view (n, r) with row stride ldu inside a NaN-filled device buffer"""
    t = eng.torch
    buf, off, ldu = layout_buffer(U, layout)
    d = eng.to_device(buf, dtype=t.float32 if buf.dtype == np.float32 else t.float64)
    return d.as_strided(U.shape, (ldu, 1), d.storage_offset() + off)


def check_sweep(eng, st, U, cap, nrm=None):
    """what a sweep leaves besides the norms, from the device's own norms: tau and the record are the candidate model's, bit
    for bit; tau lies between the bounds that hold for any sound candidate rule; the record holds the maximum, the lowest
    row attaining it, the second-largest value and the stored row.  -> (nrm, rec, tau)"""
    n, row0 = st['n'], st['row0']
    nrm = host(eng, st['nrm']) if nrm is None else nrm
    rec, tau = host(eng, st['rec']), float(host(eng, st['tau'])[0])
    assert not np.isnan(nrm).any() and not np.isnan(rec).any()
    grid = sweep_grid(n, cap)
    cand, want_tau = candidate_model(nrm, row0, grid)
    assert bits(tau) == bits(want_tau), (tau, want_tau)
    lo, hi = tau_bounds(nrm, grid)
    assert lo <= tau <= hi, (lo, tau, hi)
    np.testing.assert_array_equal(bits(rec), bits(model_record(nrm, cand, row0, U)))
    live = np.flatnonzero(nrm >= 0)
    if live.size:                                             # the same without the model
        top = np.sort(nrm[live])[::-1]
        assert bits(rec[0]) == bits(top[0]) and rec[1] == row0 + int(np.argmax(nrm))
        assert bits(rec[2]) == bits(top[1] if live.size > 1 else -2.0)
        np.testing.assert_array_equal(bits(rec[3:]), bits(widen(U)[int(rec[1]) - row0]))
    return nrm, rec, tau


# ---- 1. init ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sweep_cases(), ids=lambda c: sweep_id(c, True))
def test_init(eng, cap, case):
    n, r, lay = case
    U = basis(n, r, f32=lay.startswith('f32'))
    Ud = upload(eng, U, lay)
    ref, bar = ref_init(U), init_bar(U)
    worst = 0.0
    for row0 in ROW0S:
        st = eng.qr_begin(Ud, row0, 1)
        nrm, rec, tau = check_sweep(eng, st, U, cap)
        worst = max(worst, float(np.max(np.abs(nrm - ref) / bar)))
        # the start from norms that already exist: the same record and bound, the given vector untouched
        given = eng.to_device(nrm)
        st2 = eng.qr_begin(Ud, row0, 1, norms=given)
        np.testing.assert_array_equal(bits(host(eng, st2['nrm'])), bits(nrm))
        np.testing.assert_array_equal(bits(host(eng, st2['rec'])), bits(rec))
        assert bits(host(eng, st2['tau'])[0]) == bits(tau)
        np.testing.assert_array_equal(bits(host(eng, given)), bits(nrm))
    print(f'init {sweep_id(case, True)}: worst error / bar = {note("init " + sweep_id(case, True), worst):.3f}')
    assert worst <= 1.0


# ---- 2. refresh with given directions ---------------------------------------------------------------------------------------
ALL_NQ_CASE = (N_TABLE, 50, 'contig')             # every nq = 1 .. 16 here, {1, 7, 16} elsewhere


def check_refresh(before, got, want, bar):
    """-> worst error / bar; rows at -1 stay -1 bit for bit (and the picked rows join them), rows at 0 stay +0"""
    assert not np.isnan(got).any()
    gone = want == -1
    np.testing.assert_array_equal(got < 0, gone)
    assert (bits(got[gone]) == bits(-1.0)).all()
    zero = (before == 0.0) & ~gone
    assert (bits(got[zero]) == bits(0.0)).all()
    assert (got[~gone] >= 0).all() and not np.signbit(got[~gone]).any()
    return float(np.max(np.abs(got - want)[~gone] / bar[~gone], initial=0.0))


@pytest.mark.parametrize('case', sweep_cases(), ids=lambda c: sweep_id(c, False))
def test_refresh(eng, cap, case):
    t = eng.torch
    n, r, lay = case
    rng = np.random.default_rng(7 * n + r)
    U = basis(n, r, f32=lay.startswith('f32'))
    Ud = upload(eng, U, lay)
    ns = min(r, 3 + QR_BATCH)
    Qh = orthonormal_rows(ns, r, r)
    st = eng.qr_begin(Ud, 0, ns)
    st['Q'].copy_(eng.to_device(Qh))
    start = eng.to_device(planted_norms(host(eng, st['nrm']), rng))
    nqs = range(1, QR_BATCH + 1) if case == ALL_NQ_CASE else (7,) if n == N_STRIDE else (1, 7, QR_BATCH)
    worst, seen = 0.0, set()
    for j0 in (0,) if n == N_STRIDE else (0, 3):
        for nq in nqs:
            nq = min(nq, r - j0)
            if nq < 1 or (j0, nq) in seen:
                continue
            seen.add((j0, nq))
            st['row0'] = row0 = ROW0S[(len(seen) + (j0 > 0)) % 2]
            picks = refresh_picks(n, row0, nq, rng)
            st['piv'][j0:j0 + nq] = eng.to_device(picks, dtype=t.int64)
            st['nrm'].copy_(start)
            before = host(eng, st['nrm'])                     # the reference starts from what the device holds
            eng.qr_refresh(st, j0, nq)
            got, _, _ = check_sweep(eng, st, U, cap)
            want = ref_apply(before, U, Qh[j0:j0 + nq], picks, row0)
            worst = max(worst, check_refresh(before, got, want, apply_bar(U, nq)))
    print(f'refresh {sweep_id(case, False)}: {len(seen)} calls, worst error / bar = '
          f'{note("refresh " + sweep_id(case, False), worst):.3f}')
    assert worst <= 1.0


@pytest.mark.parametrize('r,lay', [(50, 'contig'), (48, 'f32'), (144, 'ld+1')])
@pytest.mark.parametrize('k', [1, QR_BATCH, QR_BATCH + 1])
def test_apply(eng, cap, r, lay, k):
    """qr_apply: the sweep kernel with directions and picks of the caller's; 17 directions make two calls, each with its own
    rounding on top of its input, so the bars of the two calls add"""
    t = eng.torch
    n, row0 = N_TABLE, 1000
    rng = np.random.default_rng(r + k)
    U = basis(n, r, f32=lay.startswith('f32'))
    st = eng.qr_begin(upload(eng, U, lay), row0, 1)
    st['nrm'].copy_(eng.to_device(planted_norms(host(eng, st['nrm']), rng)))
    before = host(eng, st['nrm'])
    dirs, picks = orthonormal_rows(k, r, k), refresh_picks(n, row0, k, rng)
    eng.qr_apply(st, eng.to_device(dirs), eng.to_device(picks, dtype=t.int64))
    got, _, _ = check_sweep(eng, st, U, cap)
    bar = apply_bar(U, min(k, QR_BATCH)) + (apply_bar(U, k - QR_BATCH) if k > QR_BATCH else 0)
    worst = check_refresh(before, got, ref_apply(before, U, dirs, picks, row0), bar)
    print(f'apply r{r}-{lay}-k{k}: worst error / bar = {note(f"apply r{r}-{lay}-k{k}", worst):.3f}')
    assert worst <= 1.0


# ---- 3. exact bases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('spot', EXACT_SPOTS)
@pytest.mark.parametrize('r', EXACT_R)
@pytest.mark.parametrize('n', EXACT_N)
def test_exact_bases(eng, cap, n, r, spot, f32):
    U, p, count = exact_basis(n, r, spot, f32)
    Ud = upload(eng, U, 'f32' if f32 else 'contig')
    res = exact_residuals(U)
    for row0 in ROW0S:
        st = eng.qr_begin(Ud, row0, 2)
        nrm, rec, _ = check_sweep(eng, st, U, cap)
        assert (bits(nrm) == bits(float(r))).all()
        assert rec[1] == row0 and bits(rec[2]) == bits(rec[0])        # an all-way tie over lanes, waves and workgroups
        eng.qr_steps(st, 0, 1)
        assert int(host(eng, st['piv'])[0]) == row0 and host(eng, st['gap'])[0] == 0.0 and host(eng, st['ok'])[0] == 1.0
        np.testing.assert_array_equal(bits(host(eng, st['Q'])[0]), bits(widen(U)[0] / np.sqrt(r)))
        eng.qr_refresh(st, 0, 1)
        nrm, rec, _ = check_sweep(eng, st, U, cap)
        np.testing.assert_array_equal(bits(nrm), bits(res))
        assert rec[0] == r and rec[1] == row0 + p
        assert (rec[2] == rec[0]) == (count > 1)
        eng.qr_steps(st, 1, 1)
        assert int(host(eng, st['piv'])[1]) == row0 + p


# ---- 4. steps, one at a time, and 7. repeatability --------------------------------------------------------------------------
TRACES = {}


def run_calls(eng, r, stepwise):
    """The driver's protocol on step_basis(r): calls of STEP_CALLS steps (then QR_BATCH), the certified prefix accepted, a
    refresh.  stepwise: every step through spr_qr_step_f64 with the record read before it; else spr_qr_steps_f64.
    -> list of dicts, everything the calls wrote"""
    U = step_basis(r)
    s = step_count(r)
    st = eng.qr_begin(eng.to_device(np.array(U)), STEP_ROW0, s)
    calls, j, sizes = [], 0, list(STEP_CALLS)
    nrm = host(eng, st['nrm'])
    while j < s:
        nb = min(sizes.pop(0) if sizes else QR_BATCH, s - j)
        c = dict(j=j, nb=nb, nrm=nrm, rec=host(eng, st['rec']), tau=host(eng, st['tau']), recs=[])
        if stepwise:
            for t in range(nb):
                c['recs'].append(host(eng, st['rec']))
                eng.qr_step(st, j + t, st['rec'][None], st['tau'][None], first=(t == 0))
        else:
            eng.qr_steps(st, j, nb)
        c.update(piv=host(eng, st['piv'])[j:j + nb].copy(), gap=host(eng, st['gap'])[j:j + nb].copy(),
                 ok=host(eng, st['ok'])[j:j + nb].copy(), Q=host(eng, st['Q'])[:j + nb].copy(), rec_steps=host(eng, st['rec']))
        k = nb if c['ok'].all() else int(np.argmin(c['ok']))
        assert k >= 1
        eng.qr_refresh(st, j, k)
        nrm = host(eng, st['nrm'])
        c.update(k=k, nrm_after=nrm, rec_after=host(eng, st['rec']), tau_after=host(eng, st['tau']))
        calls.append(c)
        j += k
    return calls


def trace(eng, r, key):
    if (r, key) not in TRACES:
        TRACES[(r, key)] = run_calls(eng, r, stepwise=(key == 'stepwise'))
    return TRACES[(r, key)]


def same_bits(a, b):
    assert len(a) == len(b)
    for ca, cb in zip(a, b):
        assert (ca['j'], ca['nb'], ca['k']) == (cb['j'], cb['nb'], cb['k'])
        for key in ('nrm', 'rec', 'tau', 'piv', 'gap', 'ok', 'Q', 'rec_steps', 'nrm_after', 'rec_after', 'tau_after'):
            np.testing.assert_array_equal(bits(ca[key]) if ca[key].dtype == np.float64 else ca[key],
                                          bits(cb[key]) if cb[key].dtype == np.float64 else cb[key], err_msg=f'{key} at step {ca["j"]}')


@pytest.mark.parametrize('r', ALL_R, ids=lambda r: f'r{r}-{step_family(r)}')
def test_steps(eng, eng2, cap, r):
    U = step_basis(r)
    grid = sweep_grid(N_TABLE, cap)
    q_bar = 8 * np.array(twin_worst()) + r * U_RND
    twin = twin_direction_errors(r)
    calls = trace(eng2, r, 'stepwise')
    worst_q, worst_gap, worst_nrm, worst_rec, tail = np.zeros(3), 0.0, 0.0, 0.0, False
    for c in calls:
        j, nb, k = c['j'], c['nb'], c['k']
        m = model_batch(c['nrm'], U, STEP_ROW0, grid, c['Q'][:j], nb, True)
        upto = min(k + 1, nb)                                 # the accepted steps and the refused one (decisive on the host)
        np.testing.assert_array_equal(c['piv'][:upto], m['piv'][:upto])
        np.testing.assert_array_equal(c['ok'][:upto], np.asarray(m['ok'][:upto], dtype=np.float64))
        assert k == (nb if all(m['ok']) else m['ok'].index(False))
        tail |= k < nb
        for t in range(upto):
            want = ref_step(c['recs'][t][None], c['tau'], t == 0, c['Q'][:j + t])       # on the device's own record
            assert int(c['piv'][t]) == want['piv'] and bool(c['ok'][t]) == want['ok']
            assert bool(c['ok'][t]) == (t == 0 or c['recs'][t][0] > c['tau'][0])
            err = abs(LD(c['gap'][t]) - want['gap'])
            worst_gap = max(worst_gap, float(err / (GAP_BAR * want['gap'])) if want['gap'] > 0 else float(err > 0))
            np.testing.assert_array_equal(bits(c['recs'][t][3:]), bits(U[int(c['piv'][t]) - STEP_ROW0]))
            worst_q = np.maximum(worst_q, direction_errors(c['Q'], j + t, c['recs'][t][3:]))
        if k == nb and record_is_decided(m):                  # the record the steps leave: the best remaining candidate
            rs = c['rec_steps']
            assert rs[1] == m['rec_row']
            np.testing.assert_array_equal(bits(rs[3:]), bits(U[m['rec_row'] - STEP_ROW0]))
            # its values: the candidates down-dated by the device's own nb directions (only the steps' rounding is measured)
            cand = candidate_model(c['nrm'], STEP_ROW0, grid)[0]
            left = np.sort(ref_apply(c['nrm'], U, c['Q'][j:j + nb], c['piv'], STEP_ROW0)[cand])[::-1]
            bar = float(apply_bar(U, nb)[cand].max())
            worst_rec = max(worst_rec, float(abs(LD(rs[0]) - left[0])) / bar, float(abs(LD(rs[2]) - left[1])) / bar)
        # the refresh applies the k accepted directions and nothing of the discarded steps
        want = ref_apply(c['nrm'], U, c['Q'][j:j + k], c['piv'][:k], STEP_ROW0)
        worst_nrm = max(worst_nrm, check_refresh(c['nrm'], c['nrm_after'], want, apply_bar(U, k)))
        cand, tau = candidate_model(c['nrm_after'], STEP_ROW0, grid)
        assert bits(c['tau_after'][0]) == bits(tau)
        np.testing.assert_array_equal(bits(c['rec_after']), bits(model_record(c['nrm_after'], cand, STEP_ROW0, U)))
    assert tail or r < 16                                     # a batch with an uncertified tail was among the calls
    print(f'steps r{r} {step_family(r)}: calls (j, nb, k) {[(c["j"], c["nb"], c["k"]) for c in calls]}')
    print(f'  |q - ref| device {worst_q[0]:.2e} double {twin[0]:.2e}   ||q| - 1| device {worst_q[1]:.2e} double {twin[1]:.2e}   '
          f'|Q q| device {worst_q[2]:.2e} double {twin[2]:.2e}   bars {q_bar[0]:.2e} {q_bar[1]:.2e} {q_bar[2]:.2e}')
    ratios = dict(q=worst_q[0] / q_bar[0], unit=worst_q[1] / q_bar[1], orth=worst_q[2] / q_bar[2], gap=worst_gap,
                  refresh=worst_nrm, rec=worst_rec)
    print('  worst error / bar: ' + '  '.join(f'{k} {note(f"steps r{r} {k}", v):.3f}' for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    # the batched entry point takes the same steps: identical bits
    same_bits(trace(eng, r, 'batched'), calls)


@pytest.mark.parametrize('r', ALL_R, ids=lambda r: f'r{r}-{step_family(r)}')
def test_steps_repeat_bit_for_bit(eng, r):
    """two runs from fresh states: the last-workgroup merge of the fused step must not depend on arrival order"""
    same_bits(run_calls(eng, r, stepwise=False), trace(eng, r, 'batched'))


# ---- 5. certification on a planted basis ------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', PLANT_R)
def test_planted_second_pivot_is_refused(eng, cap, r):
    case = planted_basis(r)
    check_planted(case)
    U = case['U']
    nb = min(QR_BATCH, r)
    Ud = eng.to_device(np.array(U))
    st = eng.qr_begin(Ud, 0, nb)
    nrm, rec, tau = check_sweep(eng, st, U, cap)
    assert 81.0 <= tau <= 121.0 and bits(tau) == bits(candidate_model(nrm, 0, sweep_grid(len(U), cap))[1])
    eng.qr_steps(st, 0, nb)
    ok = host(eng, st['ok'])
    assert ok[0] == 1.0 and ok[1] == 0.0
    # the mirror: the first step certified against tau like the others -- strictly above it
    st = eng.qr_begin(Ud, 0, nb)
    eng.qr_steps(st, 0, nb, first_exact=False)
    assert rec[0] > tau and host(eng, st['ok'])[0] == 1.0
    clipped = np.minimum(nrm, tau)                            # every row above the TOPT-th best of tau's workgroup comes down to it
    for bump, want in ((False, 0.0), (True, 1.0)):
        given = clipped.copy()
        if bump:
            given[int(np.argmax(nrm))] = np.nextafter(tau, np.inf)
        st = eng.qr_begin(Ud, 0, nb, norms=eng.to_device(given))
        rec2, tau2 = host(eng, st['rec']), host(eng, st['tau'])[0]
        assert bits(tau2) == bits(tau) and bits(rec2[0]) == bits(given.max())
        eng.qr_steps(st, 0, nb, first_exact=False)
        assert host(eng, st['ok'])[0] == want, (bump, rec2[0], tau2)
        st = eng.qr_begin(Ud, 0, nb, norms=eng.to_device(given))
        eng.qr_steps(st, 0, nb, first_exact=True)
        assert host(eng, st['ok'])[0] == 1.0


@pytest.mark.parametrize('pools', [False, True])
@pytest.mark.parametrize('r', PLANT_R + (PLANT_R_POOLS,))
def test_planted_pivot_loop(eng, r, pools):
    case = planted_basis(r)
    want = check_planted(case)
    st = eng.qr_begin(eng.to_device(np.array(case['U'])), 0, case['s'])
    if pools and r == PLANT_R_POOLS:
        assert eng.qr_epoch_ok(st)
    sweeps = pivot_loop(eng, st, case['s'], pools=pools)
    np.testing.assert_array_equal(host(eng, st['piv'])[:case['s']], want)
    assert sweeps >= 2                                        # the refused second step forced a sweep


# ---- 6. two shards on one device --------------------------------------------------------------------------------------------
def run_shards(eng, eng2, U, n1, s, swap=False, batch=4):
    t = eng.torch
    st1 = eng.qr_begin(eng.to_device(U[:n1].copy()), 0, s)
    st2 = eng2.qr_begin(eng2.to_device(U[n1:].copy()), n1, s)
    j = 0
    while j < s:
        nb = min(batch, s - j)
        taus = t.stack([st1['tau'], st2['tau']])
        for i in range(nb):
            recs = t.stack([st2['rec'], st1['rec']] if swap else [st1['rec'], st2['rec']])
            eng.qr_step(st1, j + i, recs, taus, first=(i == 0))
            eng2.qr_step(st2, j + i, recs, taus, first=(i == 0))
        ok = host(eng, st1['ok'])[j:j + nb]
        k = nb if ok.all() else int(np.argmin(ok))
        assert k >= 1
        eng.qr_refresh(st1, j, k)
        eng2.qr_refresh(st2, j, k)
        j += k
    return st1, st2


@pytest.mark.parametrize('tie', [False, True], ids=['plain', 'tie-across-the-split'])
@pytest.mark.parametrize('n1', SHARD_SPLITS)
@pytest.mark.parametrize('r', SHARD_R)
def test_two_shards(eng, eng2, r, n1, tie):
    U = np.array(shard_basis(r, tie))
    s = shard_steps(r)
    st1, st2 = run_shards(eng, eng2, U, n1, s, swap=tie)
    for key in ('piv', 'ok', 'gap', 'Q'):                     # identical inputs: identical bits
        a, b = host(eng, st1[key]), host(eng2, st2[key])
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b)
    piv = host(eng, st1['piv'])
    want, _ = greedy_pivots_ld(U, s)
    np.testing.assert_array_equal(piv, want)
    single = eng.qr_begin(eng.to_device(U), 0, s)
    pivot_loop(eng, single, s)
    np.testing.assert_array_equal(host(eng, single['piv']), want)
    if tie:
        assert piv[0] == 40 and host(eng, st1['gap'])[0] == 0.0          # the lower global row of the two equal records
    nrm1, nrm2 = host(eng, st1['nrm']), host(eng2, st2['nrm'])
    np.testing.assert_array_equal(np.flatnonzero(nrm1 < 0), np.sort(piv[piv < n1]))
    np.testing.assert_array_equal(np.flatnonzero(nrm2 < 0) + n1, np.sort(piv[piv >= n1]))
    assert (bits(nrm1[nrm1 < 0]) == bits(-1.0)).all() and (bits(nrm2[nrm2 < 0]) == bits(-1.0)).all()


@pytest.mark.parametrize('r', SHARD_R)
def test_the_other_shards_tau_refuses_a_step(eng, eng2, r):
    """ok = best > max(taus): with first = 0 the winner must be STRICTLY above the larger bound, whichever shard it is from"""
    t = eng.torch
    U = np.array(shard_basis(r))
    n1 = 100
    for own, other, want in ((-2.0, 0.0, 0.0), (-2.0, -1.0, 1.0), (0.0, -2.0, 0.0), (-1.0, -2.0, 1.0)):
        st1 = eng.qr_begin(eng.to_device(U[:n1].copy()), 0, 1)
        st2 = eng2.qr_begin(eng2.to_device(U[n1:].copy()), n1, 1)
        recs = t.stack([st1['rec'], st2['rec']])
        rh = host(eng, recs)
        w = int(np.lexsort((rh[:, 1], -rh[:, 0]))[0])
        best = rh[w, 0]
        val = {0.0: best, -1.0: np.nextafter(best, 0.0), -2.0: -2.0}      # equal to the winner, one ulp below it, no bound
        taus = np.array([[val[own]], [val[other]]] if w == 0 else [[val[other]], [val[own]]])
        td = eng.to_device(taus)
        eng.qr_step(st1, 0, recs, td, first=False)
        eng2.qr_step(st2, 0, recs, td, first=False)
        assert host(eng, st1['ok'])[0] == want and host(eng2, st2['ok'])[0] == want, (own, other)
        assert host(eng, st1['piv'])[0] == int(rh[w, 1]) == host(eng2, st2['piv'])[0]
        eng.qr_step(st1, 0, recs, td, first=True)                          # first = 1 certifies whatever the bounds
        assert host(eng, st1['ok'])[0] == 1.0


def test_zz_worst_ratio_overall():
    if WORST:
        k = max(WORST, key=WORST.get)
        print(f'pivot kernels, worst error / bar over {len(WORST)} toleranced cases: {WORST[k]:.3f} in {k}')
        for fam in ('init', 'refresh', 'apply', 'steps'):
            sub = {t: v for t, v in WORST.items() if t.startswith(fam)}
            if sub:
                kk = max(sub, key=sub.get)
                print(f'  {fam}: {sub[kk]:.3f} in {kk}')
        assert WORST[k] <= 1.0

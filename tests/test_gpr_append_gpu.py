"""spr_gp_state_f64 / spr_gp_append_f64 (csrc/gp.hip, engine.gp_state / gp_append) on the GPU against the longdouble oracle of
tests/test_gpr_append_host.py, at the smallest shapes where the kernels can go wrong.  The edges are the block row of 16, the LDS
chunk of 32, the 64 x 32 tiles of the W step, the 256 column owners, k = 1 and k = 64, and the limit m' = 800: (m_old, k) in
{(1, 1), (2, 1), (37, 1), (37, 17), (64, 16), (65, 64), (130, 2), (256, 1), (257, 64), (530, 17), (736, 64), (799, 1)}, d in {1, 3},
r in {1, 5}, flags 0..3, all four kernels at m_old = 37, Y and V with a row stride, w a mix of 0 and 1 (append_case of the host
file: every third old point and every other new one carry a given variance).

THE BAR is that of tests/test_gpr_gpu.py, unchanged: rel = 16 m' eps kappa_2(K') with K' from the longdouble oracle, times the norm
bounds |K'^-1|_2 for K'^-1, |K'^-1|_2 |res|_2 for alpha, (sa |res| / 2 + sum |log r_jj^2| / 2 + m' log(2 pi) / 2) / m' for the loss; logdet is
held to rel sum |log r_jj^2|.  Inputs are chosen so that rel < 1e-8 (asserted; computed on the CPU from the oracle's K' alone): modes
take the raw settings q % 3 of tests/test_gpr_ard_host.py, the cases with m' >= 547 (r = 1) the settings 0 or 1 -- setting 2, the
long lengthscale, gives rel = 1.1e-8 .. 2.1e-8 there.  The two cases with m' = 800 share one data set and one longdouble evaluation
(8 s on the CPU), the split into old and new rows is all that differs.  The cases with one or two points carry an output scale:
without it their pivots are 1 + n, log det K' is about 0.03, and rel sum |log r_jj^2| falls below the half ulp that rounding K's own
entries puts into a logarithm (the float64 oracle misses that bar too); with o != 1 the logarithms are of order 1."""
import functools

import numpy as np
import pytest

from openmeasure_amd.gpr import GPR, GPKernel
from tests.test_gpr_ard_gpu import strided
from tests.test_gpr_ard_host import scaled_t, split, widen
from tests.test_gpr_append_host import append_bars, append_case, append_errors, chain_case, gp_state_oracle
from tests.test_gpr_host import KERNELS, field_case, gp_kernel

pytestmark = pytest.mark.gpu
LD = np.longdouble
F64 = lambda a: np.asarray(a, dtype=np.float64)


@pytest.fixture(scope='module')
def eng():
    from openmeasure_amd.engine import HipEngine
    return HipEngine('cuda:0')


@functools.lru_cache(maxsize=None)
def reference(m_tot, d, r, flags, kernel, seed, setting):
    """the data of a case (the old / new split only says which rows carry which noise pattern: it is part of the seed's case) and
    the longdouble evaluation of every mode, with its bar.  setting: None (mode q takes q % 3) or the one setting of all modes"""
    m, k = seed
    P0, Y, w, V = append_case(m, k, d, r, seed=m_tot)
    raws = np.array([widen(q % 3 if setting is None else setting, d, flags) for q in range(r)])
    evs = []
    for q in range(r):
        ev = gp_state_oracle(P0, Y[:, q], raws[q], kernel, flags, w, V[:, q], dtype=LD)
        rel, sc = append_bars(ev, m_tot)
        assert rel < 1e-8, rel
        evs.append((ev, rel, sc))
    return P0, Y, w, V, raws, evs


def host(eng, *ts):
    return [eng.to_host(t) for t in ts]


def check_against(tag, got, evs):
    """got: per mode dicts with Kinv, alpha, logdet, loss -> asserts each within rel x its scale, prints the worst ratio"""
    for q, (g, (ev, rel, sc)) in enumerate(zip(got, evs)):
        errs = append_errors(g, ev)
        print(f'{tag} mode {q}: bar {rel:.2e} errors / scale ' + ' '.join(f'{k} {v / max(sc[k], 1e-300):.2e}' for k, v in errs.items()))
        for key, e in errs.items():
            assert e <= rel * sc[key], (tag, q, key, e, rel, sc[key])


# ------------------------------------------------------------------------------------------------ gp_state
@pytest.mark.parametrize('m,r,flags', [(1, 5, 2), (1, 5, 3)] + [(m, r, f) for m, r in ((37, 5), (130, 1), (257, 1)) for f in range(4)])
def test_state_is_the_factorisation_of_gp_train_noise(eng, m, r, flags):
    d, kernel = 3, 'matern52'
    P0, Y, w, V = (a[:m] for a in append_case(m, 1, d, r, seed=m))
    raws = np.array([widen(q % 3, d, flags) for q in range(r)])
    args = (eng.to_device(P0), strided(eng, Y), eng.to_device(w), strided(eng, V, pad=2), kernel, flags)
    raw_d = eng.to_device(raws)
    _, Kinv0, alpha0, info0, _ = eng.gp_train_noise(*args, raw_d, 0.1, 0, 0.0)
    Kinv, alpha, info, X, logdet = eng.gp_state(*args, raw_d)
    Kinv0, alpha0, info0, Kinv, alpha, info, X, logdet, raw_after = host(eng, Kinv0, alpha0, info0, Kinv, alpha, info, X, logdet, raw_d)
    assert np.array_equal(Kinv, Kinv0) and np.array_equal(alpha, alpha0) and np.array_equal(info, info0, equal_nan=True) and np.all(info[:, 3] == 0)      # (e is NaN without a step)
    assert np.array_equal(raw_after, raws) and X.shape == (r, m, m) and logdet.shape == (r,)
    for q in range(r):
        ev = gp_state_oracle(P0, Y[:, q], raws[q], kernel, flags, w, V[:, q], dtype=LD)
        rel, sc = append_bars(ev, m)
        assert rel < 1e-8
        assert np.all(np.triu(X[q], 1) == 0)
        assert np.max(np.abs(X[q].T @ X[q] - ev['Kinv'])) <= rel * sc['Kinv']
        assert abs(logdet[q] - ev['logdet']) <= rel * sc['logdet']


# ------------------------------------------------------------------------------------------------ gp_append
APPEND_CASES = [(1, 1, 1, 5, 2, None), (2, 1, 3, 1, 3, None), (37, 1, 1, 5, 0, None), (37, 17, 3, 5, 1, None), (64, 16, 3, 1, 0, None),
                (65, 64, 1, 5, 3, None), (130, 2, 3, 5, 0, None), (256, 1, 3, 1, 2, None), (257, 64, 3, 1, 1, None),
                (530, 17, 3, 1, 3, 1), (736, 64, 3, 1, 0, 0), (799, 1, 3, 1, 0, 0)]
APPEND_PARAMS = [c + (kernel,) for c in APPEND_CASES for kernel in (KERNELS if c[0] == 37 else ('matern52',))]


@pytest.mark.parametrize('m,k,d,r,flags,setting,kernel', APPEND_PARAMS)
def test_append_against_the_longdouble_oracle(eng, m, k, d, r, flags, setting, kernel):
    """a gp_state of the first m rows, one gp_append of the last k: K'^-1, alpha', logdet' and the loss against the longdouble
    evaluation of all m + k rows at the bar; the structure of X'; symmetry; the inputs untouched; a second run with the same bits"""
    mp = m + k
    P0, Y, w, V, raws, evs = reference(mp, d, r, flags, kernel, (736, 64) if mp == 800 else (m, k), setting)
    P0_d, Y_d, w_d, V_d, raw_d = eng.to_device(P0), strided(eng, Y), eng.to_device(w), strided(eng, V, pad=2), eng.to_device(raws)
    Kinv, alpha, info, X, logdet = eng.gp_state(P0_d[:m], Y_d[:m], w_d[:m], V_d[:m], kernel, flags, raw_d)
    assert np.all(eng.to_host(info)[:, 3] == 0)
    before = host(eng, X, Kinv, logdet, raw_d)
    runs = [host(eng, *eng.gp_append(P0_d, Y_d, w_d, V_d, kernel, flags, raw_d, X, Kinv, logdet, k)) for _ in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(before, host(eng, X, Kinv, logdet, raw_d)))       # the old state is never written
    assert all(np.array_equal(a, b) for a, b in zip(*runs))                                          # two runs, the same bits
    X2, Kinv2, alpha2, logdet2, info2 = runs[0]
    assert X2.shape == Kinv2.shape == (r, mp, mp) and alpha2.shape == (r, mp) and info2.shape == (r, 4)
    assert np.all(info2[:, 0] == mp) and np.all(info2[:, 3] == 0) and np.array_equal(info2[:, 2], logdet2)
    for q in range(r):
        assert np.array_equal(X2[q][:m, :m], before[0][q]) and np.all(X2[q][:m, m:] == 0) and np.all(np.triu(X2[q], 1) == 0)
        assert np.array_equal(Kinv2[q], Kinv2[q].T)
        ev, rel, sc = evs[q]
        assert np.max(np.abs(X2[q].T @ X2[q] - ev['Kinv'])) <= rel * sc['Kinv']
    check_against(f'append m={m} k={k} d={d} flags={flags} {kernel}',
                  [dict(Kinv=Kinv2[q], alpha=alpha2[q], logdet=logdet2[q], loss=info2[q, 1]) for q in range(r)], evs)


def test_a_chain_of_twelve_appends(eng):
    """k = 3 from m = 37 on the near-duplicate inputs of the host file's chain (d = 1, s2 = 1e-4, V = 1e-8 on the new points, every
    third one 1e-7 from an earlier point): the end of the chain against a fresh gp_state of all 73 points and against the
    longdouble oracle, both at the bar (its formula; kappa is about 1e9 here, the cap on rel does not apply)."""
    P0, y, w, v, raw = chain_case(n_steps=36)
    m, n = 37, 73
    P0_d, Y_d, w_d, V_d = eng.to_device(P0), strided(eng, y[:, None]), eng.to_device(w), strided(eng, v[:, None], pad=2)
    raw_d = eng.to_device(raw[None, :])
    Kinv, alpha, info, X, logdet = eng.gp_state(P0_d[:m], Y_d[:m], w_d[:m], V_d[:m], 'matern52', 0, raw_d)
    for m_end in range(m + 3, n + 1, 3):
        X, Kinv, alpha, logdet, info = eng.gp_append(P0_d[:m_end], Y_d[:m_end], w_d[:m_end], V_d[:m_end], 'matern52', 0, raw_d, X, Kinv,
                                                     logdet, 3)
    fresh = eng.gp_state(P0_d, Y_d, w_d, V_d, 'matern52', 0, raw_d)
    Kinv, alpha, info, X, logdet, fKinv, falpha, finfo, fX, flogdet = host(eng, Kinv, alpha, info, X, logdet, *fresh)
    assert info[0, 3] == 0 and finfo[0, 3] == 0 and info[0, 0] == n and np.array_equal(Kinv[0], Kinv[0].T)
    ev = gp_state_oracle(P0, y, raw, 'matern52', 0, w, v, dtype=LD)
    rel, sc = append_bars(ev, n)
    got = dict(Kinv=Kinv[0], alpha=alpha[0], logdet=logdet[0], loss=info[0, 1])
    check_against('chain', [got], [(ev, rel, sc)])
    diff = dict(Kinv=np.max(np.abs(Kinv[0] - fKinv[0])), alpha=np.max(np.abs(alpha[0] - falpha[0])), logdet=abs(logdet[0] - flogdet[0]),
                loss=abs(info[0, 1] - finfo[0, 1]))
    print(f'chain against a fresh state: bar {rel:.2e} (kappa {np.linalg.cond(F64(ev["K"])):.2e}) differences / scale ' +
          ' '.join(f'{k} {v / sc[k]:.2e}' for k, v in diff.items()))
    for key, e in diff.items():
        assert e <= rel * sc[key], (key, e, rel, sc[key])


def test_a_copy_of_an_exact_point_stops_its_mode_only(eng):
    """The new point equals old point 5; both are exact (w = 0, V = 0) in mode 2 of 5 and carry a variance in the others: K' of mode
    2 is singular, its Schur complement a few eps of either sign -- status 1 for that mode alone, the other four within the bar,
    the inputs unchanged."""
    m, k, d, r, flags, kernel = 37, 1, 3, 5, 0, 'matern52'
    P0, Y, w, V = append_case(m, k, d, r, seed=77)
    P0[m] = P0[5]
    w[5] = w[m] = 0.0
    V[5], V[m] = 0.04, 0.09
    V[5, 1] = V[m, 1] = 0.0
    raws = np.array([widen(q % 3, d, flags) for q in range(r)])
    P0_d, Y_d, w_d, V_d, raw_d = eng.to_device(P0), strided(eng, Y), eng.to_device(w), strided(eng, V, pad=2), eng.to_device(raws)
    Kinv, alpha, info, X, logdet = eng.gp_state(P0_d[:m], Y_d[:m], w_d[:m], V_d[:m], kernel, flags, raw_d)
    assert np.all(eng.to_host(info)[:, 3] == 0)
    before = host(eng, X, Kinv, logdet, raw_d, P0_d, Y_d, w_d, V_d)
    X2, Kinv2, alpha2, logdet2, info2 = host(eng, *eng.gp_append(P0_d, Y_d, w_d, V_d, kernel, flags, raw_d, X, Kinv, logdet, k))
    assert all(np.array_equal(a, b) for a, b in zip(before, host(eng, X, Kinv, logdet, raw_d, P0_d, Y_d, w_d, V_d)))
    assert info2[:, 3].tolist() == [0, 1, 0, 0, 0] and np.isnan(info2[1, 1]) and np.isnan(logdet2[1])
    for q in (0, 2, 3, 4):
        ev = gp_state_oracle(P0, Y[:, q], raws[q], kernel, flags, w, V[:, q], dtype=LD)
        rel, sc = append_bars(ev, m + k)
        assert rel < 1e-8
        check_against(f'beside a failed mode, mode {q}', [dict(Kinv=Kinv2[q], alpha=alpha2[q], logdet=logdet2[q], loss=info2[q, 1])],
                      [(ev, rel, sc)])


# ------------------------------------------------------------------------------------------------ GPR
@pytest.mark.parametrize('kernel', [None, GPKernel('matern52', ard=True, scale=True)], ids=['plain', 'ard+scale'])
def test_end_to_end_three_appends_against_one_fixed_noise_update(eng, kernel):
    """fit / train on field_case, then update(append=True) three times (1, 3 and 70 points) against one update(fixed_noise=True)
    with all 74 on a second object trained the same way (training is deterministic: the same hyper-parameters, bit for bit).  Both
    K'^-1 / alpha are within rel of the truth, so predict's mean and variance differ by at most 2 rel times the sums of absolute
    terms of tests/test_gpr_gpu.py's predict test with o in them: |mu| + o |k*|_2 sa and o + o^2 |k*|_2^2 sK + s2."""
    flags = 0 if kernel is None else kernel.flags
    X, F, P = field_case()
    objs = []
    for _ in range(2):
        g = GPR(X, F, None, P, engine=eng)
        g.fit(select_modes='number', n_modes=3)
        g.train(kernel=kernel, max_iter=30, rel_error=0.0)
        objs.append(g)
    g, h = objs
    assert all(np.array_equal(a.raw, b.raw) for a, b in zip(g.models, h.models))
    rng = np.random.default_rng(2)
    Pn = np.column_stack([1.0 + 3.0 * rng.random(74), 300 + 50 * rng.random(74)])
    amax = np.abs(g.Ar).max()
    An = g.predict(Pn)[0] + 0.02 * amax * rng.standard_normal((74, 3))
    Sn = 0.02 * amax * (0.5 + rng.random((74, 3)))
    for a, b in ((0, 1), (1, 4), (4, 74)):
        g.update(Pn[a:b], An[a:b], Sn[a:b], append=True)
    h.update(Pn, An, Sn, fixed_noise=True)
    assert g.gpr_info_['n_train'] == h.gpr_info_['n_train'] == 86 and g.gpr_info_['n_added'] == 74
    assert [s['rows'] for s in g.append_info_] == [64, 6] and g.Vr_sigma.shape == (86, 3)
    P_star = np.array([[2.2, 320.0], [3.3, 341.0], P[4], Pn[7]])
    (A1, S1), (A2, S2) = g.predict(P_star), h.predict(P_star)
    P0_tot, Y_tot = eng.to_host(h._d['gp_P0']), eng.to_host(h._d['gp_Y'])
    assert np.array_equal(eng.to_host(g._d['gp_P0']), P0_tot) and np.array_equal(eng.to_host(g._d['gp_Y']), Y_tot)
    w, V = h.gpr_info_['noise_weight'], h.gpr_info_['fixed_noise']
    Ps0 = (P_star - g.P_cnt[0]) / g.P_scl[0]
    Sig = np.asarray(g.Sigma_r)
    for q, rec in enumerate(h.models):
        ev = gp_state_oracle(P0_tot, Y_tot[:, q], rec.raw, 'matern52', flags, w, V[:, q], dtype=LD)
        rel, sc = append_bars(ev, 86)
        ell, o, s2, mu = (F64(a) for a in split(rec.raw, 2, flags))
        kn = np.linalg.norm(gp_kernel('matern52', scaled_t(Ps0 / ell, P0_tot / ell)[0])[0], axis=1)
        em = np.abs(A1[:, q] - A2[:, q]) / Sig[q] / (abs(mu) + o * kn * sc['alpha'])
        evr = np.abs((S1[:, q] / Sig[q]) ** 2 - (S2[:, q] / Sig[q]) ** 2) / (o + o * o * kn * kn * sc['Kinv'] + s2)
        print(f'end to end mode {q}: 2 x bar {2 * rel:.2e} mean {np.max(em):.2e} variance {np.max(evr):.2e} '
              f'loss {abs(g.gpr_info_["loss"][q] - h.gpr_info_["loss"][q]) / sc["loss"]:.2e}')
        assert np.all(em <= 2 * rel) and np.all(evr <= 2 * rel)
        assert abs(g.gpr_info_['loss'][q] - h.gpr_info_['loss'][q]) <= 2 * rel * sc['loss']
    field = g.reconstruct(A1)
    assert field.shape == (X.shape[0], 4) and np.all(np.isfinite(field)) and np.all(np.isfinite(g.reconstruct_std(S1)))

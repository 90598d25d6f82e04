"""Differential check of the host logic against the reference, through its RECORDED outcomes: oracle/make_reference_record.py
ran the unmodified reference on the inputs below and stored what it returned or raised in tests/golden/reference_outcomes.json
(values, shapes, dtypes, exception types and texts, method signatures).  The product's classes run over the NumPy test double of
the kernels, so what is compared is everything around the kernels: rank selection, the top-r eigen route of fit() (m >= 96),
exception types and messages, shapes and dtypes -- on inputs the golden fixtures do not cover (m >= 96, 'variance' thresholds,
Fortran-ordered / float32 / integer X).  The inputs are regenerated here from their seeds; the record also stores a fingerprint
of each (shape, dtype, sum, norm: BLAS builds round the generator's product differently in the last bits), so a change of the
generator cannot pass unnoticed."""
import inspect
import json
import os
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'reference_outcomes.json')


@pytest.fixture(scope='module')
def rec():
    with open(RECORD) as f:
        return json.load(f)


def mine_ns():
    """the product's ROM / SPR over the NumPy test double, called the way the reference's classes are"""
    from openmeasure_amd.sparse_sensing import ROM, SPR
    from tests.numpy_engine import NumpyEngine
    return types.SimpleNamespace(SPR=lambda *a, **k: SPR(*a, engine=NumpyEngine(), **k),
                                 ROM=lambda *a, **k: ROM(*a, engine=NumpyEngine(), **k))


def _data(n_points, F, m, k, rho, seed, dtype=np.float64, order='C'):
    rng = np.random.default_rng(seed)
    n = n_points * F
    X = rng.standard_normal((n, k)) @ ((rho ** np.arange(k))[:, None] * rng.standard_normal((k, m))) + 1e-3 * rng.standard_normal((n, m))
    for f in range(F):
        X[f * n_points:(f + 1) * n_points] = (f + 1) * X[f * n_points:(f + 1) * n_points] + 10.0 * f
    return np.asarray(X, dtype=dtype, order=order)


def fingerprint(a):
    """shape, dtype, sum and norm of an input array"""
    a = np.asarray(a)
    w = a.astype(np.float64)
    return [list(a.shape), str(a.dtype), float(w.sum()), float(np.linalg.norm(w))]


def same_input(fp_mine, fp_ref):
    """the fingerprints of the same input: shape and dtype exact, sum and norm to the rounding of the generator"""
    return fp_mine[:2] == fp_ref[:2] and np.allclose(fp_mine[2:], fp_ref[2:], rtol=1e-9, atol=0)


def floats(a):
    return [float(v) for v in np.ravel(a)]


def outcome_of(fn):
    """('ok', None) or (exception type name, text)"""
    try:
        fn()
    except Exception as exc:                                  # noqa: BLE001 -- whatever the reference raises is the specification
        return [type(exc).__name__, str(exc)]
    return ['ok', None]


FIT_CASES = [(128, 'number', 16, np.float64, 'C'), (160, 'variance', 99.0, np.float64, 'C'), (100, 'variance', 99.9, np.float64, 'F'),
             (128, 'number', 60, np.float32, 'C'), (96, 'variance', 100, np.float64, 'C'), (130, 'number', 90, np.float64, 'C'),
             (128, 'variance', 50.0, np.float64, 'C')]


def fit_key(m, select, n_modes, dtype, order):
    return f'{m}-{select}-{n_modes!r}-{np.dtype(dtype).name}-{order}'


def fit_input(m, dtype, order):
    return _data(300, 2, m, 40, 0.8, seed=m, dtype=dtype, order=order)


def fit_measurements(X, piv, n_points=300):
    y = np.zeros((len(piv), 3))
    y[:, 0] = np.asarray(X, dtype=np.float64)[piv, 3]
    y[:, 2] = piv // n_points
    return y


def record_fit(ns, m, select, n_modes, dtype, order):
    """what test_fit_place_predict_reconstruct_matches_the_reference reads of a reference object"""
    X = fit_input(m, dtype, order)
    ref = ns.SPR(X.copy(order=order), 2, None)
    ref.fit(select_modes=select, n_modes=n_modes)
    out = dict(X_fingerprint=fingerprint(X), r=int(ref.r), Sigma_r=floats(ref.Sigma_r), Ur_shape=list(ref.Ur.shape), Ar_shape=list(ref.Ar.shape),
               Ur_dtype=str(ref.Ur.dtype))
    if ref.r == m:
        return out
    C_ref = ref.optimal_placement()
    piv = np.argmax(C_ref, axis=1)
    ref.train(C_ref)
    a_ref, _ = ref.predict(fit_measurements(X, piv))
    x_ref = ref.reconstruct(a_ref)
    out.update(piv=[int(p) for p in piv], x_shape=list(x_ref.shape), x=floats(x_ref))
    return out


@pytest.mark.parametrize('m,select,n_modes,dtype,order', FIT_CASES)
def test_fit_place_predict_reconstruct_matches_the_reference(rec, m, select, n_modes, dtype, order):
    ref = rec['fit'][fit_key(m, select, n_modes, dtype, order)]
    X = fit_input(m, dtype, order)
    assert same_input(fingerprint(X), ref['X_fingerprint']), 'the input is not the one the reference was run on'
    mine = mine_ns().SPR(X.copy(order=order), 2, None)
    mine.fit(select_modes=select, n_modes=n_modes)
    assert mine.r == ref['r']
    keep = mine.r - 1 if mine.r == m else mine.r              # the null mode of a full-rank row-centred fit is rounding noise in both
    np.testing.assert_allclose(mine.Sigma_r[:keep], np.array(ref['Sigma_r'])[:keep], rtol=2e-6 if dtype == np.float32 else 1e-8)
    assert list(mine.Ur.shape) == ref['Ur_shape'] and list(mine.Ar.shape) == ref['Ar_shape'] and str(mine.Ur.dtype) == ref['Ur_dtype']
    if mine.r == m:
        return
    C = mine.optimal_placement()
    piv = np.array(ref['piv'])
    if dtype == np.float64:                                   # float32 input: the reference's own means are float32-rounded
        np.testing.assert_array_equal(np.argmax(np.asarray(C), axis=1), piv)
    mine.train(C)
    if dtype == np.float64:
        a, s_ = mine.predict(fit_measurements(X, piv))
        x = mine.reconstruct(a)
        x_ref = np.array(ref['x']).reshape(ref['x_shape'])
        assert x.shape == x_ref.shape
        assert np.linalg.norm(x - x_ref) <= 1e-6 * np.linalg.norm(x_ref)


FIT_ERRORS = [(dict(scale_type='vast_3'), ValueError), (dict(select_modes='number', n_modes=0), ValueError),
              (dict(select_modes='number', n_modes=2.0), TypeError), (dict(select_modes='variance', n_modes=101), ValueError),
              (dict(select_modes='bogus'), ValueError), (dict(scale_type='bogus'), NotImplementedError)]


def error_input():
    return _data(60, 2, 100, 10, 0.7, seed=1)


def record_fit_error(ns, kw):
    return outcome_of(lambda: ns.SPR(error_input(), 2, None).fit(**kw))


@pytest.mark.parametrize('kw,exc', FIT_ERRORS)
def test_fit_errors_match_the_reference(rec, kw, exc):
    e_ref = rec['fit_errors'][repr(sorted(kw.items()))]
    assert e_ref[0] == exc.__name__
    with pytest.raises(exc) as e_mine:
        mine_ns().SPR(error_input(), 2, None).fit(**kw)
    if exc is ValueError and 'scale_type' in kw:
        assert str(e_mine.value) == e_ref[1]                  # NumPy's broadcast message, shapes included


AXIS_CNTS = [0, 2, -1, -2, 7, -3]


def axis_input():
    return _data(60, 2, 12, 6, 0.7, seed=2)


def record_axis_cnt(ns, axis_cnt):
    ref = ns.SPR(axis_input(), 2, None)
    out = dict(outcome=outcome_of(lambda: ref.fit(axis_cnt=axis_cnt, select_modes='number', n_modes=3)))
    if out['outcome'][0] == 'ok':
        out.update(X_cnt=floats(ref.X_cnt), X_cnt_shape=list(np.shape(ref.X_cnt)), Sigma_r=floats(ref.Sigma_r))
    return out


@pytest.mark.parametrize('axis_cnt', AXIS_CNTS)
def test_axis_cnt_values_behave_like_the_reference(rec, axis_cnt):
    """round 6: axis_cnt goes to np.average(x, axis=axis_cnt) (:112) -- whatever the reference does with a
    value (row means for -1, NumPy's broadcast ValueError for 0 / -2, its AxisError beyond), type AND text, happens here too."""
    ref = rec['axis_cnt'][str(axis_cnt)]
    mine = mine_ns().SPR(axis_input(), 2, None)
    if ref['outcome'][0] == 'ok':
        mine.fit(axis_cnt=axis_cnt, select_modes='number', n_modes=3)
        np.testing.assert_allclose(mine.X_cnt, np.array(ref['X_cnt']).reshape(ref['X_cnt_shape']), rtol=1e-13)
        np.testing.assert_allclose(mine.Sigma_r, ref['Sigma_r'], rtol=1e-9)
    else:
        with pytest.raises(Exception) as e_mine:
            mine.fit(axis_cnt=axis_cnt, select_modes='number', n_modes=3)
        assert [type(e_mine.value).__name__, str(e_mine.value)] == ref['outcome']


def record_misshaped_sampling(ns):
    o = ns.SPR(_data(10, 2, 5, 4, 0.7, seed=3), 2, None)
    o.fit(select_modes='number', n_modes=3)
    return [outcome_of(lambda: o.reconstruct(np.zeros(3), sampling=np.eye(19))),
            outcome_of(lambda: o.unscale_data(np.zeros(19), sampling=np.eye(19)))]


def test_misshaped_sampling_matrix_raises_numpys_text(rec):
    ref = rec['misshaped_sampling']
    assert [e[0] for e in ref] == ['ValueError', 'ValueError']
    assert record_misshaped_sampling(mine_ns()) == ref


def record_attributes(ns):
    rng = np.random.default_rng(3)
    X, xyz = rng.random((40, 6)), rng.random((20, 3))
    o = ns.SPR(X.copy(), 2, xyz)
    o.fit(select_modes='number', n_modes=4)
    C = o.optimal_placement()
    o.train(C, cond=True)
    piv = np.argmax(np.asarray(C), axis=1)
    y = np.zeros((4, 3))
    y[:, 0] = X[piv, 0]
    y[:, 2] = piv // 20
    o.predict(y)
    return o


def attribute_record(o):
    out = {}
    for name in sorted(vars(o)):
        a = getattr(o, name)
        if isinstance(a, np.ndarray):
            out[name] = dict(shape=list(a.shape), dtype=str(a.dtype))
        elif isinstance(a, (int, str, bool)) or a is None:
            out[name] = dict(value=a)
        else:
            out[name] = {}
    return dict(attributes=out, k=float(o.k))


def test_every_attribute_of_a_used_reference_object_exists_here(rec):
    """After fit -> optimal_placement -> train(cond=True) -> predict the reference object carries 22 instance attributes
    (X, X0, X_cnt, X_scl, Ur, Ar, Vr, Sigma_r, r, C, Theta, cnt_vector, scl_vector, k, limits, method, solver, verbose, ...):
    each of them can be read from the product's object, with the same shape and dtype (values: the fixture tests)."""
    ref = rec['attributes']
    mine = record_attributes(mine_ns())
    assert len(ref['attributes']) >= 22
    for name, want in ref['attributes'].items():
        assert hasattr(mine, name), name
        b = getattr(mine, name)
        if 'shape' in want:
            b = np.asarray(b)
            assert list(b.shape) == want['shape'] and str(b.dtype) == want['dtype'], name
        elif 'value' in want:
            assert want['value'] == b, name
    assert abs(ref['k'] - mine.k) <= 1e-12 * ref['k']


def record_signatures(module):
    """{class: {public method: [[parameter name, repr of its default (None: no default), kind], ...]}}"""
    out = {}
    for cls in ('ROM', 'SPR'):
        out[cls] = {}
        for name, f in inspect.getmembers(getattr(module, cls), inspect.isfunction):
            if name.startswith('_') and name != '__init__':
                continue
            out[cls][name] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default), p.kind.name]
                              for p in inspect.signature(f).parameters.values()]
    return out


def test_every_public_method_of_the_reference_exists_with_its_signature(rec):
    """names, parameter names, order and defaults of every public method of ROM and SPR (extra trailing keyword parameters
    are allowed: shard=, engine=, to_host=, wait=); CPOD and adaptive_sampling exist and raise NotImplementedError."""
    import openmeasure_amd.sparse_sensing as mine
    for cls, methods in rec['signatures'].items():
        M = getattr(mine, cls)
        assert methods, cls
        for name, pr in methods.items():
            g = getattr(M, name)
            pm = list(inspect.signature(g).parameters.values())
            assert len(pm) >= len(pr), (cls, name)
            for a, b in zip(pr, pm):
                got = [b.name, None if b.default is inspect.Parameter.empty else repr(b.default), b.kind.name]
                assert got == a, (cls, name, a, got)
            for extra in pm[len(pr):]:
                assert extra.default is not inspect.Parameter.empty, (cls, name, extra)
    from tests.numpy_engine import NumpyEngine
    o = mine.SPR(np.zeros((4, 2)), 2, None, engine=NumpyEngine())
    with pytest.raises(NotImplementedError):
        o.CPOD({})
    with pytest.raises(NotImplementedError):
        o.adaptive_sampling(np.zeros((2, 1)))


def _differential_cases(ns):
    """-> {name: outcome} with the classes of `ns` (ns.SPR / ns.ROM called like the reference's); an outcome is
    ['ok', repr of the value] or [exception type name, repr of its text, cut at 160 characters]"""
    rng=np.random.default_rng(0)
    def data(n_points=30,F=2,m=8):
        X=rng.standard_normal((n_points*F,4))@rng.standard_normal((4,m))+0.01*rng.standard_normal((n_points*F,m))
        X[n_points:]+=5
        return X
    def run(make, steps):
        try:
            o=make()
            res=None
            for st in steps:
                res=st(o)
            return ['ok', repr(res)]
        except Exception as e:
            return [type(e).__name__, repr(str(e)[:160])]
    X=data(); xyz=rng.random((30,3))
    def mk(X=X, F=2, xyz=xyz):
        return ns.SPR(X.copy(),F,xyz)
    def mkrom(X=X, F=2, xyz=xyz):
        return ns.ROM(X.copy(),F,xyz)
    cases={'inputs': ['ok', [fingerprint(X), fingerprint(xyz)]]}
    cases['ctor list']=run(lambda:ns.SPR([[1,2],[3,4]],2,None),[])
    cases['ctor F float']=run(lambda:ns.SPR(X,2.0,None),[])
    cases['ctor F bool']=run(lambda:ns.SPR(X,True,None),[])
    cases['ctor not multiple']=run(lambda:ns.SPR(X[:59],2,None),[])
    cases['ctor 1-D X']=run(lambda:ns.SPR(X[:,0].copy(),2,None),[lambda o:o.fit()])
    cases['ctor 3-D X']=run(lambda:ns.SPR(np.zeros((4,2,2)),2,None),[lambda o:o.fit()])
    cases['ctor F=0']=run(lambda:ns.SPR(X,0,None),[])
    for nm in (True, 1, 8, 9, 0, -1, 3.0, '3', None):
        cases[f'fit number {nm!r}']=run(mk,[lambda o,nm=nm:(o.fit(select_modes='number',n_modes=nm), o.r)[1]])
    for nm in (0, 100, 99.999, -1, 100.5, 50, '50', None, True):
        cases[f'fit variance {nm!r}']=run(mk,[lambda o,nm=nm:(o.fit(select_modes='variance',n_modes=nm), o.r)[1]])
    cases['fit select None']=run(mk,[lambda o:o.fit(select_modes=None)])
    cases['fit basis tuple']=run(mk,[lambda o:(o.fit(basis=(np.eye(60,3),np.eye(8,3))), o.r, o.Sigma_r.tolist())[1:]])
    cases['fit basis bad']=run(mk,[lambda o:o.fit(basis=(np.eye(60,3),))])
    cases['fit basis mismatched r']=run(mk,[lambda o:(o.fit(basis=(np.eye(60,3),np.eye(8,4))), o.r)[1]])
    fit=lambda o:o.fit(select_modes='number',n_modes=3)
    cases['placement bogus']=run(mk,[fit,lambda o:o.optimal_placement(calc_type='bogus')])
    cases['placement before fit']=run(mk,[lambda o:o.optimal_placement()])
    cases['placement mask wrong len']=run(mk,[fit,lambda o:o.optimal_placement(mask=np.ones(10,bool)).shape])
    cases['placement mask int']=run(mk,[fit,lambda o:np.argmax(np.asarray(o.optimal_placement(mask=np.ones(60,int))),axis=1).tolist()])
    cases['placement mask all false']=run(mk,[fit,lambda o:np.asarray(o.optimal_placement(mask=np.zeros(60,bool))).shape])
    cases['placement n_sensors ignored']=run(mk,[fit,lambda o:np.asarray(o.optimal_placement(n_sensors=1)).shape])
    cases['train wrong cols']=run(mk,[fit,lambda o:o.train(np.eye(3,59))])
    cases['train before fit']=run(mk,[lambda o:o.train(np.eye(3,60))])
    cases['train theta wrong cols']=run(mk,[fit,lambda o:o.train(np.eye(3,4),is_Theta=True)])
    cases['train theta ok']=run(mk,[fit,lambda o:(o.train(np.eye(5,3),is_Theta=True), o.Theta.shape)[1]])
    cases['train method bogus']=run(mk,[fit,lambda o:(o.train(np.eye(3,60),method='bogus'), o.method)[1]])
    cases['train 1-D C']=run(mk,[fit,lambda o:o.train(np.ones(60))])
    cases['train list C']=run(mk,[fit,lambda o:o.train(np.eye(3,60).tolist())])
    def placed(o):
        o.fit(select_modes='number',n_modes=3); C=o.optimal_placement(); o.train(C); return C
    def yvec(o,rows=3,cols=3):
        y=np.zeros((rows,cols)); y[:,0]=1.0; return y
    cases['predict wrong rows']=run(mk,[placed,lambda o:o.predict(yvec(o,4))])
    cases['predict wrong cols']=run(mk,[placed,lambda o:o.predict(yvec(o,3,2))])
    cases['predict list empty']=run(mk,[placed,lambda o:[a.shape for a in o.predict([])]])
    cases['predict method bogus']=run(mk,[lambda o:(o.fit(select_modes='number',n_modes=3), o.train(o.optimal_placement(),method='bogus'), o.predict(yvec(o)))[2]])
    cases['predict before train']=run(mk,[fit,lambda o:o.predict(yvec(o))])
    cases['predict feature id 5']=run(mk,[placed,lambda o:o.predict(np.array([[1,0,5],[1,0,0],[1,0,0.]]))])
    cases['predict feature id -1']=run(mk,[placed,lambda o:np.round(o.predict(np.array([[1,0,-1],[1,0,0],[1,0,0.]]))[0],6).shape])
    cases['predict tuple']=run(mk,[placed,lambda o:[a.shape for a in o.predict((yvec(o),))]])
    cases['predict 1-D y']=run(mk,[placed,lambda o:o.predict(np.zeros(3))])
    cases['predict after is_Theta']=run(mk,[fit,lambda o:(o.train(np.eye(3,3),is_Theta=True), o.predict(yvec(o)))[1]])
    cases['reconstruct wrong r']=run(mk,[fit,lambda o:o.reconstruct(np.zeros(4))])
    cases['reconstruct 2-D']=run(mk,[fit,lambda o:o.reconstruct(np.zeros((2,3))).shape])
    cases['reconstruct before fit']=run(mk,[lambda o:o.reconstruct(np.zeros(3))])
    cases['reconstruct list']=run(mk,[fit,lambda o:np.asarray(o.reconstruct([0.,0.,0.])).shape])
    cases['reconstruct empty']=run(mk,[fit,lambda o:o.reconstruct(np.zeros((0,3))).shape])
    cases['reconstruct sampling 1-D']=run(mk,[fit,lambda o:o.reconstruct(np.zeros(3),sampling=np.ones(60))])
    cases['unscale wrong len']=run(mk,[fit,lambda o:o.unscale_data(np.zeros(59))])
    cases['unscale list']=run(mk,[fit,lambda o:o.unscale_data([0.]*60)])
    cases['unscale before fit']=run(mk,[lambda o:o.unscale_data(np.zeros(60))])
    cases['scale_data bogus']=run(mkrom,[lambda o:o.scale_data('bogus')])
    cases['scale_limits']=run(mkrom,[lambda o:(o.scale_data(), [np.round(a[:2],6).tolist() for a in o.scale_limits([np.array([0.,1.]),np.array([2.,3.])])])[1]])
    cases['scale_limits before']=run(mkrom,[lambda o:o.scale_limits([np.array([0.,1.])])])
    cases['reduction bad select']=run(mkrom,[lambda o:o.reduction(np.eye(60,8),np.eye(8),np.linspace(50,100,8),'bogus',3)])
    cases['decomposition']=run(mkrom,[lambda o:[a.shape for a in o.decomposition(o.scale_data(),'number',3)]])
    cases['decomposition foreign X0']=run(mkrom,[lambda o:[a.shape for a in o.decomposition(np.asarray(data()),'variance',90)]])
    cases['gem n_sensors 0']=run(mk,[fit,lambda o:o.optimal_placement(calc_type='gem',n_sensors=0)])
    cases['scale_vector']=run(mk,[placed,lambda o:np.round(o.scale_vector(yvec(o)),8).tolist()])
    cases['scale_vector wrong rows']=run(mk,[placed,lambda o:o.scale_vector(yvec(o,5))])

    return cases


#: outcomes that differ ON PURPOSE (documented in the module docstring of sparse_sensing.py / INTEGRATION.md)
_KNOWN_DEVIATIONS = {
    'placement mask int',        # an integer "mask" indexes rows in the reference (Ur[~mask, :] = 0 with ~1 = -2): refused here
    'reconstruct list',          # a list of coefficients is accepted here (the reference needs an ndarray)
    'unscale list',              # the reference hands back a cvxpy expression for a non-ndarray; no such object on the device path
    'unscale wrong len',         # the text comes from cvxpy in the real reference (the fixtures' stand-in gives NumPy's, operands swapped)
}


def test_seventy_host_logic_cases_against_the_imported_reference(rec):
    """round 6: constructor / fit / optimal_placement / train / predict / reconstruct / unscale_data / scale_limits / decomposition
    called the wrong and the right way, the product's classes (over the NumPy test double) next to the reference's recorded
    outcomes: same outcome -- value, or exception TYPE AND TEXT -- in every case but the four documented deviations."""
    ref = rec['cases']
    cases = _differential_cases(mine_ns())
    assert sorted(cases) == sorted(ref)
    assert all(same_input(a, b) for a, b in zip(cases['inputs'][1], ref['inputs'][1])), \
        'the inputs are not the ones the reference was run on'
    assert len(cases) - 1 >= 70
    bad = []
    for name, b in cases.items():
        if name == 'inputs':
            continue
        a = ref[name]
        same = a == b
        if name in _KNOWN_DEVIATIONS:
            assert not same, f'{name}: no longer deviates -- take it off the list'
        elif not same:
            bad.append((name, a, b))
    assert not bad, bad

"""Refusals of the co-kriging entry points (csrc/cokriging.hip) without a GPU: status, text and order, in the manner of
tests/test_gp_args_host.py.  Every call here is refused before anything is launched; the pointers are small integers that
stand in for device addresses."""
import pytest

from openmeasure_amd import _lib

INVALID, UNSUPPORTED = -1, -2
P = [8 * (i + 1) for i in range(16)]
BIG = 1 << 40
NAN, INF = float('nan'), float('inf')

TRAIN = ('X n d ldx Y r ldy Rho ldr regr v nugget v_lo v_hi lr max_iter tol Rinv RinvF Ginv beta gamma sigma2 info trace ws ws_bytes '
         'stream',
         dict(X=P[0], n=10, d=2, ldx=2, Y=P[1], r=3, ldy=3, Rho=P[2], ldr=3, regr=1, v=P[3], nugget=1e-10, v_lo=-5.0, v_hi=1.7,
              lr=0.1, max_iter=5, tol=1e-6, Rinv=P[4], RinvF=P[5], Ginv=P[6], beta=P[7], gamma=P[8], sigma2=P[9], info=P[10],
              trace=None, ws=P[11], ws_bytes=BIG, stream=None))
PREDICT = ('X n d ldx Xstar n_p ldxs RhoStar ldrs regr v r Rinv RinvF Ginv beta gamma sigma2 mean mse stream',
           dict(X=P[0], n=10, d=2, ldx=2, Xstar=P[1], n_p=4, ldxs=2, RhoStar=P[2], ldrs=3, regr=1, v=P[3], r=3, Rinv=P[4],
                RinvF=P[5], Ginv=P[6], beta=P[7], gamma=P[8], sigma2=P[9], mean=P[10], mse=P[11], stream=None))
TABLE = {'spr_ck_train_f64': TRAIN, 'spr_ck_predict_f64': PREDICT}
T, Q = 'spr_ck_train_f64', 'spr_ck_predict_f64'

CASES = (
    [(T, {k: None}, INVALID, 'NULL') for k in ('X', 'Y', 'v', 'Rinv', 'RinvF', 'Ginv', 'beta', 'gamma', 'sigma2', 'info', 'ws')] +
    [(T, {k: 0}, INVALID, 'bad shape') for k in ('n', 'd', 'r')] +
    [(T, {'ldx': 1}, INVALID, 'bad shape'), (T, {'ldy': 2}, INVALID, 'bad shape'), (T, {'ldr': 2}, INVALID, 'bad shape'),
     (T, {'max_iter': -1}, INVALID, 'bad shape'),
     (T, {'Rho': None, 'ldr': 0}, INVALID, 'workspace of'),         # no rho column: ldr is not looked at (refused later, by the workspace)
     (T, {'regr': 2}, INVALID, 'regr code'), (T, {'regr': -1}, INVALID, 'regr code'),
     (T, {'n': 4}, INVALID, 'do not exceed the 4 trend columns'),   # rho, 1, two coordinates
     (T, {'n': 4, 'Rho': None}, INVALID, 'workspace of'),           # ... three columns without rho: n = 4 will do
     (T, {'n': 2, 'regr': 0}, INVALID, 'do not exceed the 2 trend columns'),
     (T, {'nugget': -1e-12}, INVALID, 'nugget'), (T, {'nugget': NAN}, INVALID, 'nugget'), (T, {'nugget': INF}, INVALID, 'nugget'),
     (T, {'lr': 0.0}, INVALID, 'lr'), (T, {'lr': NAN}, INVALID, 'lr'), (T, {'tol': -1.0}, INVALID, 'tol'), (T, {'tol': INF}, INVALID, 'tol'),
     (T, {'v_lo': 2.0}, INVALID, 'bounds'), (T, {'v_lo': NAN}, INVALID, 'bounds'), (T, {'v_hi': INF}, INVALID, 'bounds'),
     (T, {'v_lo': -INF}, INVALID, 'bounds'),
     (T, {'n': 801}, UNSUPPORTED, 'exceeds 800'), (T, {'d': 9, 'ldx': 9, 'n': 20}, UNSUPPORTED, 'coordinates exceed 8'),
     (T, {'ws_bytes': 'one short'}, INVALID, 'workspace of'), (T, {'ws': 12}, INVALID, '8-byte aligned'),
     # order: pointers, shape, regr code, trend columns, nugget / step / tolerance / bounds, the caps, the workspace
     (T, {'X': None, 'n': 0}, INVALID, 'NULL'), (T, {'n': 0, 'regr': 9}, INVALID, 'bad shape'), (T, {'regr': 9, 'nugget': -1.0}, INVALID, 'regr code'),
     (T, {'nugget': -1.0, 'lr': 0.0}, INVALID, 'nugget'), (T, {'lr': 0.0, 'v_lo': 9.0}, INVALID, 'lr'), (T, {'v_lo': 9.0, 'n': 801}, INVALID, 'bounds'),
     (T, {'n': 801, 'ws_bytes': 0}, UNSUPPORTED, 'exceeds 800'), (T, {'ws_bytes': 0, 'ws': 12}, INVALID, 'workspace of')] +
    [(Q, {k: None}, INVALID, 'NULL') for k in ('X', 'Xstar', 'v', 'Rinv', 'RinvF', 'Ginv', 'beta', 'gamma', 'sigma2', 'mean', 'mse')] +
    [(Q, {k: 0}, INVALID, 'bad shape') for k in ('n', 'd', 'r', 'n_p')] +
    [(Q, {'ldx': 1}, INVALID, 'bad shape'), (Q, {'ldxs': 1}, INVALID, 'bad shape'), (Q, {'ldrs': 2}, INVALID, 'bad shape'),
     (Q, {'regr': 2}, INVALID, 'regr code'), (Q, {'n': 4}, INVALID, 'do not exceed the 4 trend columns'),
     (Q, {'n': 801}, UNSUPPORTED, 'exceeds 800'), (Q, {'d': 9, 'ldx': 9, 'ldxs': 9, 'n': 20}, UNSUPPORTED, 'coordinates exceed 8'),
     (Q, {'n_p': 8 * 65535 + 1}, UNSUPPORTED, 'test points per call'),
     (Q, {'mse': None, 'n_p': 0}, INVALID, 'NULL'), (Q, {'n_p': 0, 'regr': 7}, INVALID, 'bad shape'), (Q, {'regr': 7, 'n': 801}, INVALID, 'regr code')])


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0][4:] + '-' + '+'.join(f'{k}={v}' for k, v in c[1].items()))
def test_refusal(case):
    entry, change, status, fragment = case
    lib = _lib.load()
    names, good = TABLE[entry]
    args = dict(good, **change)
    if fragment == 'workspace of' and 'ws_bytes' not in change:
        args['ws_bytes'] = 0                                     # every earlier check passed: the workspace is the first refusal
    if args.get('ws_bytes') == 'one short':
        need = lib.spr_ck_workspace(args['n'], args['d'], args['r'])
        assert need == 8 * args['r'] * (2 * args['n'] ** 2 + args['n'] * args['d'])
        args['ws_bytes'] = need - 1
    rc = getattr(lib, entry)(*[args[n] for n in names.split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith(entry + ': ') and fragment in text, text


def test_workspace_function_refuses_shapes_the_entry_refuses():
    lib = _lib.load()
    assert lib.spr_ck_workspace(0, 2, 3) == 0 and lib.spr_ck_workspace(10, 0, 3) == 0 and lib.spr_ck_workspace(10, 2, 0) == 0
    assert lib.spr_ck_workspace(801, 2, 1) == 0 and lib.spr_ck_workspace(10, 9, 1) == 0
    assert lib.spr_ck_workspace(800, 8, 1) == 8 * (2 * 800 * 800 + 800 * 8)


def test_the_trend_cap_is_the_coordinate_cap_plus_two():
    assert _lib.SPR_CK_MAX_P == _lib.SPR_GP_MAX_D + 2 == 10

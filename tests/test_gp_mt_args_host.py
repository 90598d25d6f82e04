"""Refusals of the multitask Gaussian-process entry points (csrc/gp.hip: spr_gp_train_mt_f64, spr_gp_predict_mt_f64,
spr_gp_workspace_mt) without a GPU: status, text and order, in the manner of tests/test_gp_args_host.py.  Every call here is
refused before anything is launched; the pointers are small integers that stand in for device addresses."""
import os
import re

import pytest

from openmeasure_amd import _lib

INVALID, UNSUPPORTED = -1, -2
P = [8 * (i + 1) for i in range(10)]
BIG = 1 << 40
T, Q = 'spr_gp_train_mt_f64', 'spr_gp_predict_mt_f64'

TRAIN = ('P0 m d ldp Y r ldy kernel flags raw raw_g lr max_iter tol s2 Kinv alpha info trace ws ws_bytes stream',
         dict(P0=P[0], m=10, d=2, ldp=2, Y=P[1], r=3, ldy=3, kernel=0, flags=3, raw=P[2], raw_g=P[7], lr=0.1, max_iter=5, tol=1e-5,
              s2=P[8], Kinv=P[3], alpha=P[4], info=P[5], trace=None, ws=P[6], ws_bytes=BIG, stream=None))
PREDICT = ('P0 m d ldp Pstar n_p ldps kernel flags raw s2 r Kinv alpha mean var stream',
           dict(P0=P[0], m=10, d=2, ldp=2, Pstar=P[1], n_p=4, ldps=2, kernel=0, flags=3, raw=P[2], s2=P[7], r=3, Kinv=P[3],
                alpha=P[4], mean=P[5], var=P[6], stream=None))
TABLE = {T: TRAIN, Q: PREDICT}
D9 = {'d': 9, 'ldp': 9}

CASES = [
    (T, {'P0': None}, INVALID, 'NULL'), (T, {'Y': None}, INVALID, 'NULL'), (T, {'raw': None}, INVALID, 'NULL'),
    (T, {'raw_g': None}, INVALID, 'NULL'), (T, {'s2': None}, INVALID, 'NULL'),
    (T, {'Kinv': None}, INVALID, 'NULL'), (T, {'alpha': None}, INVALID, 'NULL'), (T, {'info': None}, INVALID, 'NULL'),
    (T, {'ws': None}, INVALID, 'NULL'),
    (T, {'m': 0}, INVALID, 'bad shape'), (T, {'d': 0}, INVALID, 'bad shape'), (T, {'r': 0}, INVALID, 'bad shape'),
    (T, {'m': -3}, INVALID, 'bad shape'), (T, {'r': -1}, INVALID, 'bad shape'),
    (T, {'ldp': 1}, INVALID, 'bad shape'), (T, {'ldy': 2}, INVALID, 'bad shape'), (T, {'max_iter': -1}, INVALID, 'bad shape'),
    (T, {'kernel': 4}, INVALID, 'kernel code'), (T, {'kernel': -1}, INVALID, 'kernel code'),
    (T, {'flags': 4}, INVALID, 'flags'), (T, {'flags': -1}, INVALID, 'flags'),
    (T, {'lr': 0.0}, INVALID, 'lr'), (T, {'lr': float('nan')}, INVALID, 'lr'),
    (T, {'tol': -1.0}, INVALID, 'tol'), (T, {'tol': float('inf')}, INVALID, 'tol'),
    (T, {'m': 801}, UNSUPPORTED, 'exceeds 800'),
    (T, dict(D9, flags=1), UNSUPPORTED, 'd = 9 coordinates exceeds 8'), (T, dict(D9, flags=3), UNSUPPORTED, 'exceeds 8'),
    (T, dict(D9, flags=2, ws_bytes='one short'), INVALID, 'workspace of'),     # the scale alone has no cap on d
    (T, dict(d=8, ldp=8, flags=3, ws_bytes='one short'), INVALID, 'workspace of'),
    (T, {'ws_bytes': 'one short'}, INVALID, 'workspace of'), (T, {'ws': 12}, INVALID, '8-byte aligned'),
    (T, {'ws_bytes': 'ard'}, INVALID, 'workspace of'),                         # the single-task workspace has no room for the state
    # order: pointers, shape, kernel code, flags, step and tolerance, the caps on m and d, the workspace
    (T, {'P0': None, 'm': 0}, INVALID, 'NULL'), (T, {'m': 0, 'kernel': 9}, INVALID, 'bad shape'),
    (T, {'kernel': 9, 'flags': 7}, INVALID, 'kernel code'), (T, {'flags': 7, 'lr': 0.0}, INVALID, 'flags'),
    (T, {'lr': 0.0, 'm': 801}, INVALID, 'lr'), (T, dict(D9, flags=1, lr=0.0), INVALID, 'lr'),
    (T, dict(D9, flags=1, m=801), UNSUPPORTED, 'exceeds 800'),
    (T, {'m': 801, 'ws_bytes': 0}, UNSUPPORTED, 'exceeds 800'), (T, dict(D9, flags=1, ws_bytes=0), UNSUPPORTED, 'exceeds 8'),
    (Q, {'P0': None}, INVALID, 'NULL'), (Q, {'Pstar': None}, INVALID, 'NULL'), (Q, {'raw': None}, INVALID, 'NULL'),
    (Q, {'s2': None}, INVALID, 'NULL'),
    (Q, {'Kinv': None}, INVALID, 'NULL'), (Q, {'alpha': None}, INVALID, 'NULL'), (Q, {'mean': None}, INVALID, 'NULL'),
    (Q, {'var': None}, INVALID, 'NULL'),
    (Q, {'m': 0}, INVALID, 'bad shape'), (Q, {'n_p': 0}, INVALID, 'bad shape'), (Q, {'r': 0}, INVALID, 'bad shape'),
    (Q, {'n_p': -4}, INVALID, 'bad shape'),
    (Q, {'ldps': 1}, INVALID, 'bad shape'), (Q, {'ldp': 1}, INVALID, 'bad shape'), (Q, {'kernel': 4}, INVALID, 'kernel code'),
    (Q, {'flags': 4}, INVALID, 'flags'), (Q, {'flags': -2}, INVALID, 'flags'),
    (Q, {'m': 801}, UNSUPPORTED, 'exceeds 800'), (Q, dict(D9, ldps=9, flags=1), UNSUPPORTED, 'd = 9 coordinates exceeds 8'),
    (Q, {'n_p': 8 * 65535 + 1}, UNSUPPORTED, 'test points per call'),
    (Q, {'var': None, 'n_p': 0}, INVALID, 'NULL'), (Q, {'n_p': 0, 'kernel': 5}, INVALID, 'bad shape'),
    (Q, {'kernel': 5, 'flags': 9}, INVALID, 'kernel code'), (Q, {'flags': 9, 'm': 801}, INVALID, 'flags'),
    (Q, dict(D9, ldps=9, flags=3, m=801), UNSUPPORTED, 'exceeds 800'),
]


def mt_workspace(m, d, r):
    """bytes: r slices (A, X, Z), the head (8), Adam's two moments (r (d + 3) + 1 each), the records (r x (d + 6)), m ones"""
    return 8 * (r * (2 * m * m + m * d) + 8 + 2 * (r * (d + 3) + 1) + r * (d + 6) + m)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0][7:] + '-' + '+'.join(f'{k}={v}' for k, v in c[1].items()))
def test_refusal(case):
    entry, change, status, fragment = case
    lib = _lib.load()
    names, good = TABLE[entry]
    args = dict(good, **change)
    if args.get('ws_bytes') == 'one short':
        need = lib.spr_gp_workspace_mt(args['m'], args['d'], args['r'])
        assert need == mt_workspace(args['m'], args['d'], args['r'])
        args['ws_bytes'] = need - 1
    elif args.get('ws_bytes') == 'ard':
        args['ws_bytes'] = lib.spr_gp_workspace_ard(args['m'], args['d'], args['r'])
    rc = getattr(lib, entry)(*[args[n] for n in names.split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith(entry + ': ') and fragment in text, text


def test_workspace_function_refuses_shapes_the_entry_refuses():
    lib = _lib.load()
    assert lib.spr_gp_workspace_mt(0, 3, 3) == 0 and lib.spr_gp_workspace_mt(10, 3, 0) == 0
    assert lib.spr_gp_workspace_mt(10, 0, 3) == 0 and lib.spr_gp_workspace_mt(801, 1, 1) == 0
    assert lib.spr_gp_workspace_mt(-1, 3, 3) == 0 and lib.spr_gp_workspace_mt(10, 3, -2) == 0
    assert lib.spr_gp_workspace_mt(800, 8, 1) == mt_workspace(800, 8, 1)
    assert lib.spr_gp_workspace_mt(10, 20, 90) == mt_workspace(10, 20, 90)          # d has a cap under ARD only: the entry's check
    assert lib.spr_gp_workspace_mt(10, 2, 3) > lib.spr_gp_workspace_ard(10, 2, 3)


def test_constants_are_mirrored():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'spr_hip.h')).read()
    assert int(re.search(r'#define SPR_GP_MT_CHUNK (\d+)', header).group(1)) == _lib.SPR_GP_MT_CHUNK
    from openmeasure_amd.engine import HipEngine
    assert HipEngine.GP_MT_CHUNK == _lib.SPR_GP_MT_CHUNK >= 2
    assert int(re.search(r'#define SPR_ABI_VERSION (\d+)', header).group(1)) == 5

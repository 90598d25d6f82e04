"""Refusals of the Gaussian-process entry points (csrc/gp.hip) without a GPU: status, text and order, in the manner of
tests/test_launch_args_host.py.  Every call here is refused before anything is launched; the pointers are small integers
that stand in for device addresses."""
import pytest

from openmeasure_amd import _lib

INVALID, UNSUPPORTED = -1, -2
P = [8 * (i + 1) for i in range(10)]
BIG = 1 << 40

TRAIN = ('P0 m d ldp Y r ldy kernel raw lr max_iter tol Kinv alpha info trace ws ws_bytes stream',
         dict(P0=P[0], m=10, d=2, ldp=2, Y=P[1], r=3, ldy=3, kernel=0, raw=P[2], lr=0.1, max_iter=5, tol=1e-5, Kinv=P[3],
              alpha=P[4], info=P[5], trace=None, ws=P[6], ws_bytes=BIG, stream=None))
PREDICT = ('P0 m d ldp Pstar n_p ldps kernel raw r Kinv alpha mean var stream',
           dict(P0=P[0], m=10, d=2, ldp=2, Pstar=P[1], n_p=4, ldps=2, kernel=0, raw=P[2], r=3, Kinv=P[3], alpha=P[4],
                mean=P[5], var=P[6], stream=None))
TABLE = {'spr_gp_train_f64': TRAIN, 'spr_gp_predict_f64': PREDICT}

CASES = [
    ('spr_gp_train_f64', {'P0': None}, INVALID, 'NULL'), ('spr_gp_train_f64', {'Y': None}, INVALID, 'NULL'),
    ('spr_gp_train_f64', {'raw': None}, INVALID, 'NULL'), ('spr_gp_train_f64', {'Kinv': None}, INVALID, 'NULL'),
    ('spr_gp_train_f64', {'alpha': None}, INVALID, 'NULL'), ('spr_gp_train_f64', {'info': None}, INVALID, 'NULL'),
    ('spr_gp_train_f64', {'ws': None}, INVALID, 'NULL'),
    ('spr_gp_train_f64', {'m': 0}, INVALID, 'bad shape'), ('spr_gp_train_f64', {'d': 0}, INVALID, 'bad shape'),
    ('spr_gp_train_f64', {'r': 0}, INVALID, 'bad shape'), ('spr_gp_train_f64', {'ldp': 1}, INVALID, 'bad shape'),
    ('spr_gp_train_f64', {'ldy': 2}, INVALID, 'bad shape'), ('spr_gp_train_f64', {'max_iter': -1}, INVALID, 'bad shape'),
    ('spr_gp_train_f64', {'kernel': 4}, INVALID, 'kernel code'), ('spr_gp_train_f64', {'kernel': -1}, INVALID, 'kernel code'),
    ('spr_gp_train_f64', {'lr': 0.0}, INVALID, 'lr'), ('spr_gp_train_f64', {'lr': float('nan')}, INVALID, 'lr'),
    ('spr_gp_train_f64', {'tol': -1.0}, INVALID, 'tol'), ('spr_gp_train_f64', {'tol': float('inf')}, INVALID, 'tol'),
    ('spr_gp_train_f64', {'m': 801}, UNSUPPORTED, 'exceeds 800'),
    ('spr_gp_train_f64', {'ws_bytes': 'one short'}, INVALID, 'workspace of'),
    ('spr_gp_train_f64', {'ws': 12}, INVALID, '8-byte aligned'),
    # order: pointers, shape, kernel code, step and tolerance, the cap on m, the workspace
    ('spr_gp_train_f64', {'P0': None, 'm': 0}, INVALID, 'NULL'), ('spr_gp_train_f64', {'m': 0, 'kernel': 9}, INVALID, 'bad shape'),
    ('spr_gp_train_f64', {'kernel': 9, 'lr': 0.0}, INVALID, 'kernel code'), ('spr_gp_train_f64', {'lr': 0.0, 'm': 801}, INVALID, 'lr'),
    ('spr_gp_train_f64', {'m': 801, 'ws_bytes': 0}, UNSUPPORTED, 'exceeds 800'),
    ('spr_gp_predict_f64', {'P0': None}, INVALID, 'NULL'), ('spr_gp_predict_f64', {'Pstar': None}, INVALID, 'NULL'),
    ('spr_gp_predict_f64', {'raw': None}, INVALID, 'NULL'), ('spr_gp_predict_f64', {'Kinv': None}, INVALID, 'NULL'),
    ('spr_gp_predict_f64', {'alpha': None}, INVALID, 'NULL'), ('spr_gp_predict_f64', {'mean': None}, INVALID, 'NULL'),
    ('spr_gp_predict_f64', {'var': None}, INVALID, 'NULL'),
    ('spr_gp_predict_f64', {'m': 0}, INVALID, 'bad shape'), ('spr_gp_predict_f64', {'n_p': 0}, INVALID, 'bad shape'),
    ('spr_gp_predict_f64', {'r': 0}, INVALID, 'bad shape'), ('spr_gp_predict_f64', {'ldps': 1}, INVALID, 'bad shape'),
    ('spr_gp_predict_f64', {'ldp': 1}, INVALID, 'bad shape'), ('spr_gp_predict_f64', {'kernel': 4}, INVALID, 'kernel code'),
    ('spr_gp_predict_f64', {'m': 801}, UNSUPPORTED, 'exceeds 800'),
    ('spr_gp_predict_f64', {'n_p': 8 * 65535 + 1}, UNSUPPORTED, 'test points per call'),
    ('spr_gp_predict_f64', {'var': None, 'n_p': 0}, INVALID, 'NULL'), ('spr_gp_predict_f64', {'n_p': 0, 'm': 801}, INVALID, 'bad shape'),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0][4:] + '-' + '+'.join(f'{k}={v}' for k, v in c[1].items()))
def test_refusal(case):
    entry, change, status, fragment = case
    lib = _lib.load()
    names, good = TABLE[entry]
    args = dict(good, **change)
    if args.get('ws_bytes') == 'one short':
        need = lib.spr_gp_workspace(args['m'], args['r'])
        assert need == 8 * args['m'] ** 2 * (1 + 2 * args['r'])
        args['ws_bytes'] = need - 1
    rc = getattr(lib, entry)(*[args[n] for n in names.split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith(entry + ': ') and fragment in text, text


def test_workspace_function_refuses_shapes_the_entry_refuses():
    lib = _lib.load()
    assert lib.spr_gp_workspace(0, 3) == 0 and lib.spr_gp_workspace(10, 0) == 0 and lib.spr_gp_workspace(801, 1) == 0
    assert lib.spr_gp_workspace(800, 1) == 8 * 800 * 800 * 3

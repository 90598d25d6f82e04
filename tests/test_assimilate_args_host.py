"""Refusals of the assimilation entry points (csrc/assimilate.hip) without a GPU: status, text and order, in the manner of
tests/test_gp_args_host.py.  Every call here is refused before anything is launched; the pointers are small integers that
stand in for device addresses.  Order: pointers (and the choice of the prior), shape, caps, workspace."""
import pytest

from openmeasure_amd import _lib

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
P = [8 * (i + 1) for i in range(16)]
BIG = 1 << 40

NAMES = 'Theta s r cnt scale n_features y n_p a0 sigma factor q Ar Ar_std F z info ws ws_bytes stream'
DIAG = dict(Theta=P[0], s=9, r=6, cnt=P[1], scale=P[2], n_features=3, y=P[3], n_p=4, a0=P[4], sigma=P[5], factor=None, q=6,
            Ar=P[6], Ar_std=P[7], F=P[8], z=None, info=P[9], ws=None, ws_bytes=0, stream=None)
FACTOR = dict(DIAG, sigma=None, factor=P[5], q=3, z=P[10], ws=P[11], ws_bytes=BIG)

CASES = [(base, {k: None}, INVALID, 'NULL') for base in ('diag', 'factor')
         for k in ('Theta', 'cnt', 'scale', 'y', 'a0', 'Ar', 'Ar_std', 'F', 'info')] + [
    ('diag', {'sigma': None}, INVALID, 'exactly one of'), ('diag', {'factor': P[12]}, INVALID, 'exactly one of'),
    ('factor', {'factor': None}, INVALID, 'exactly one of'),
    ('diag', {'s': 0}, INVALID, 'bad shape'), ('diag', {'r': 0}, INVALID, 'bad shape'), ('diag', {'n_p': 0}, INVALID, 'bad shape'),
    ('diag', {'n_features': 0}, INVALID, 'bad shape'), ('diag', {'q': 5}, INVALID, 'bad shape'),
    ('factor', {'q': 0}, INVALID, 'bad shape'), ('factor', {'q': 7}, INVALID, 'bad shape'), ('factor', {'n_p': -1}, INVALID, 'bad shape'),
    ('diag', {'r': 129, 'q': 129}, UNSUPPORTED, 'r=129 > 128 not built'),
    ('factor', {'r': 129}, UNSUPPORTED, 'r=129 > 128 not built'),
    ('factor', {'ws': None}, INVALID, 'needs a workspace'),
    ('factor', {'ws_bytes': 'one short'}, WORKSPACE, 'workspace too small'),
    ('factor', {'ws': 12}, INVALID, '8-byte aligned'),
    # order: pointers, the choice of the prior, shape, the cap on r, the workspace
    ('diag', {'Theta': None, 'sigma': None}, INVALID, 'NULL'), ('diag', {'sigma': None, 's': 0}, INVALID, 'exactly one of'),
    ('factor', {'s': 0, 'r': 129}, INVALID, 'bad shape'), ('factor', {'q': 200, 'r': 129}, INVALID, 'bad shape'),
    ('factor', {'r': 129, 'ws_bytes': 0}, UNSUPPORTED, 'not built'), ('factor', {'r': 129, 'ws': None}, UNSUPPORTED, 'not built'),
    ('factor', {'ws': None, 'ws_bytes': 0}, INVALID, 'needs a workspace'), ('factor', {'ws_bytes': 0, 'ws': 12}, WORKSPACE, 'too small'),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0] + '-' + '+'.join(f'{k}={v}' for k, v in c[1].items()))
def test_refusal(case):
    base, change, status, fragment = case
    lib = _lib.load()
    args = dict(DIAG if base == 'diag' else FACTOR, **change)
    if args.get('ws_bytes') == 'one short':
        need = lib.spr_assimilate_workspace(args['s'], args['r'], args['q'], args['n_p'])
        assert need == 8 * args['n_p'] * args['s'] * (args['q'] + 1)
        args['ws_bytes'] = need - 1
    rc = lib.spr_assimilate_f64(*[args[n] for n in NAMES.split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith('spr_assimilate_f64: ') and fragment in text, text


def test_workspace_function_refuses_shapes_the_entry_refuses():
    ws = _lib.load().spr_assimilate_workspace
    assert ws(0, 6, 3, 4) == 0 and ws(9, 0, 1, 4) == 0 and ws(9, 6, 0, 4) == 0 and ws(9, 6, 7, 4) == 0 and ws(9, 6, 3, 0) == 0
    assert ws(9, 129, 3, 4) == 0
    assert ws(9, 128, 128, 4) == 8 * 4 * 9 * 129 and ws(4096, 32, 32, 1000) == 8 * 1000 * 4096 * 33


def test_binding_and_engine_know_the_entry_points():
    from openmeasure_amd.engine import HipEngine
    assert {'spr_assimilate_f64', 'spr_assimilate_workspace'} <= set(_lib.PROTOTYPES)
    assert callable(HipEngine.assimilate)

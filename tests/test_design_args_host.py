"""Refusals of the design-sweep entry points (csrc/design.hip) without a GPU: status, text and order, in the manner of
tests/test_cokriging_args_host.py.  Every call here is refused before anything is launched; the pointers are small integers
that stand in for device addresses."""
import pytest

from openmeasure_amd import _lib

INVALID, UNSUPPORTED = -1, -2
P = [8 * (i + 1) for i in range(8)]
BIG = 1 << 40

NAMES = 'Ur n_rows r ldu row0 n_points n_features B wfeat alive criterion scores rec ws ws_bytes stream'
GOOD = dict(Ur=P[0], n_rows=1000, r=12, ldu=12, row0=100, n_points=400, n_features=3, B=P[1], wfeat=P[2], alive=P[3],
            criterion=1, scores=P[4], rec=P[5], ws=P[6], ws_bytes=BIG, stream=None)
ENTRIES = ('spr_design_sweep_f64', 'spr_design_sweep_u32')

CASES = (
    [({k: None}, INVALID, 'NULL') for k in ('Ur', 'B', 'rec', 'ws')] +
    [({k: 0}, INVALID, 'bad shape') for k in ('n_rows', 'r')] +
    [({'n_rows': -5}, INVALID, 'bad shape'), ({'ldu': 11}, INVALID, 'bad shape'),
     ({'n_points': 0}, INVALID, 'bad feature layout'), ({'n_features': 0}, INVALID, 'bad feature layout'),
     ({'row0': -1}, INVALID, 'bad feature layout'), ({'row0': 201}, INVALID, 'bad feature layout'),
     ({'criterion': 2}, INVALID, 'criterion = 2'), ({'criterion': -1}, INVALID, 'criterion = -1'),
     ({'r': 129, 'ldu': 129}, UNSUPPORTED, 'exceeds 128'),
     ({'ws_bytes': 'one short'}, INVALID, 'workspace of'), ({'ws_bytes': 0}, INVALID, 'workspace of'),
     # order: pointers, shape, layout, criterion, the cap, the workspace
     ({'Ur': None, 'r': 0}, INVALID, 'NULL'), ({'r': 0, 'n_points': 0}, INVALID, 'bad shape'),
     ({'n_points': 0, 'criterion': 7}, INVALID, 'bad feature layout'),
     ({'criterion': 7, 'r': 129, 'ldu': 129}, INVALID, 'criterion = 7'),
     ({'r': 129, 'ldu': 129, 'ws_bytes': 0}, UNSUPPORTED, 'exceeds 128')])


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('case', CASES, ids=lambda c: '+'.join(f'{k}={v}' for k, v in c[0].items()))
def test_refusal(entry, case):
    change, status, fragment = case
    lib = _lib.load()
    args = dict(GOOD, **change)
    if args['ws_bytes'] == 'one short':
        need = lib.spr_design_sweep_workspace(args['r'], args['n_features'])
        assert need > 0 and need % 24 == 0                           # three doubles per workgroup slot
        args['ws_bytes'] = need - 1
    rc = getattr(lib, entry)(*[args[n] for n in NAMES.split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith(entry + ': ') and fragment in text, text


@pytest.mark.parametrize('entry', ENTRIES)
def test_optional_pointers_are_optional(entry):
    """wfeat, alive and scores may be NULL: with them absent the call still reaches (and fails) the workspace check"""
    lib = _lib.load()
    args = dict(GOOD, wfeat=None, alive=None, scores=None, ws_bytes=0)
    rc = getattr(lib, entry)(*[args[n] for n in NAMES.split()])
    assert rc == INVALID and 'workspace of' in lib.spr_last_error().decode()


def test_workspace_query_refuses_what_the_entry_refuses():
    lib = _lib.load()
    for r, F in ((0, 3), (-1, 3), (12, 0), (12, -2), (129, 3)):
        assert lib.spr_design_sweep_workspace(r, F) == 0
    w1, w9 = lib.spr_design_sweep_workspace(1, 1), lib.spr_design_sweep_workspace(128, 9)
    assert w1 > 0 and w9 == w1 + 8 * 24                              # one more slot per feature, whatever r


def test_prototypes_are_bound():
    assert {'spr_design_sweep_workspace', 'spr_design_sweep_f64', 'spr_design_sweep_u32'} <= set(_lib.PROTOTYPES)

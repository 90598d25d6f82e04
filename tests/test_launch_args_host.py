"""Refusals of the launchers' argument checks: status, text and order, per entry-point family.

Every call in this file is one the library refuses BEFORE it touches the device: the pointers are small integers that
stand in for device addresses, so a call that would be valid does not belong here.  The table pins what a caller sees
(status code, the entry's own name as prefix, the distinguishing words of the text) and, where two defects are present at
once, which check fires first."""
import pytest

from openmeasure_amd import _lib

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -4
P = [8 * (i + 1) for i in range(12)]     # stand-in non-NULL pointers, never dereferenced
BIG = 1 << 40                             # a workspace size no check objects to

# family -> (ordered argument names, a well-formed argument set, workspace function and its argument names, f32 twins)
FAMILIES = {
    'spr_bound_sweep_f64': (
        'Ur n_rows r ldu row0 n_points n_features rowmean scale limits clamp G n_p tol k out ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, n_points=50, n_features=2, rowmean=P[1], scale=P[2], limits=P[3],
             clamp=P[4], G=P[5], n_p=3, tol=0.0, k=2, out=P[6], ws=P[7], ws_bytes=BIG, stream=None),
        ('spr_bound_sweep_workspace', 'n_p n_features'), ['spr_bound_sweep_u32']),
    'spr_bound_sweep_batch_f64': (
        'Ur n_rows r ldu row0 n_points n_features rowmean scale limits clamp G n_p tol k out ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, n_points=50, n_features=2, rowmean=P[1], scale=P[2], limits=P[3],
             clamp=P[4], G=P[5], n_p=3, tol=0.0, k=2, out=P[6], ws=P[7], ws_bytes=BIG, stream=None),
        ('spr_bound_sweep_batch_workspace', 'n_p n_features'), ['spr_bound_sweep_batch_u32']),
    'spr_encode_f64': (
        'Ur n_rows r ldu X k ldx row0 n_points n_features rowmean scale A ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, X=P[1], k=3, ldx=3, row0=0, n_points=50, n_features=2, rowmean=P[2],
             scale=P[3], A=P[4], ws=P[5], ws_bytes=BIG, stream=None),
        ('spr_encode_workspace', 'r k n_features'), ['spr_encode_x32', 'spr_encode_u32', 'spr_encode_x32_u32']),
    'spr_field_error_f64': (
        'Ur n_rows r ldu row0 n_points n_features rowmean scale A k X ldx out ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, n_points=50, n_features=2, rowmean=P[1], scale=P[2], A=P[3], k=3,
             X=P[4], ldx=3, out=P[5], ws=P[6], ws_bytes=BIG, stream=None),
        ('spr_field_error_workspace', 'k n_features'),
        ['spr_field_error_x32', 'spr_field_error_u32', 'spr_field_error_x32_u32']),
    'spr_gappy_normal_f64': (
        'Ur n_rows r ldu X k ldx row0 n_points n_features rowmean scale mask ldm H B nobs ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, X=P[1], k=3, ldx=3, row0=0, n_points=50, n_features=2, rowmean=P[2],
             scale=P[3], mask=P[4], ldm=3, H=P[5], B=P[6], nobs=P[7], ws=P[8], ws_bytes=BIG, stream=None),
        ('spr_gappy_normal_workspace', 'r k n_features'),
        ['spr_gappy_normal_x32', 'spr_gappy_normal_u32', 'spr_gappy_normal_x32_u32']),
    'spr_gappy_fill_f64': (
        'Ur n_rows r ldu X k ldx row0 n_points n_features rowmean scale A mask ldm out ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, X=P[1], k=3, ldx=3, row0=0, n_points=50, n_features=2, rowmean=P[2],
             scale=P[3], A=P[4], mask=P[5], ldm=3, out=P[6], ws=P[7], ws_bytes=BIG, stream=None),
        ('spr_gappy_fill_workspace', ''), ['spr_gappy_fill_x32', 'spr_gappy_fill_u32', 'spr_gappy_fill_x32_u32']),
    'spr_field_std_diag_f64': (
        'Ur n_rows r ldu row0 n_points n_features scale rowscale S k out ldo stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, n_points=50, n_features=2, scale=P[1], rowscale=None, S=P[2], k=3,
             out=P[3], ldo=100, stream=None),
        None, ['spr_field_std_diag_u32']),
    'spr_field_std_factor_f64': (
        'Ur n_rows r ldu row0 n_points n_features scale rowscale S k q out ldo stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, n_points=50, n_features=2, scale=P[1], rowscale=None, S=P[2], k=3,
             q=4, out=P[3], ldo=100, stream=None),
        None, ['spr_field_std_factor_u32']),
    'spr_reconstruct_f64': (
        'Ur n_rows r ldu row0 n_points n_features rowmean scale rowscale A k out ldo stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, n_points=50, n_features=2, rowmean=P[1], scale=P[2], rowscale=None,
             A=P[3], k=3, out=P[4], ldo=100, stream=None),
        None, ['spr_reconstruct_u32']),
    'spr_project_f64': (
        'X n_rows k ldx row0 n_points n_features center inv_scale rowmean W r Ur ldu accumulate stream',
        dict(X=P[0], n_rows=100, k=3, ldx=3, row0=0, n_points=50, n_features=2, center=1, inv_scale=P[1], rowmean=P[2],
             W=P[3], r=8, Ur=P[4], ldu=8, accumulate=0, stream=None),
        None, ['spr_project_x32', 'spr_project_x32_f64out']),
}

# families whose checks differ from the pattern above (the layout is part of the shape check, other texts, other statuses):
# their refusals are listed one by one in _other_cases()
OTHER = {
    'spr_project_stream_f64': (
        'X n_rows k ldx row0 n_points n_features center inv_scale rowmean W r Ur ldu ws ws_bytes stream',
        dict(X=P[0], n_rows=100, k=3, ldx=3, row0=0, n_points=50, n_features=2, center=1, inv_scale=P[1], rowmean=P[2],
             W=P[3], r=8, Ur=P[4], ldu=8, ws=P[5], ws_bytes=BIG, stream=None),
        ('spr_project_stream_workspace', 'k r x32'), ['spr_project_stream_x32', 'spr_project_stream_x32_f64out']),
    'spr_feature_minmax_f64': (
        'X n_rows k ldx row0 n_points n_features out ws ws_bytes stream',
        dict(X=P[0], n_rows=100, k=3, ldx=3, row0=0, n_points=50, n_features=2, out=P[1], ws=P[2], ws_bytes=BIG,
             stream=None),
        ('spr_feature_minmax_workspace', 'n_features'), ['spr_feature_minmax_x32']),
    'spr_colsums_f64': (
        'X n_rows k ldx row0 n_points n_features rowmean out ws ws_bytes stream',
        dict(X=P[0], n_rows=100, k=3, ldx=3, row0=0, n_points=50, n_features=2, rowmean=P[1], out=P[2], ws=P[3],
             ws_bytes=BIG, stream=None),
        ('spr_colsums_workspace', 'k n_features'), ['spr_colsums_x32']),
    'spr_rowstats_f64': (
        'X n_rows k ldx row0 n_points n_features rowmean out ws ws_bytes stream',
        dict(X=P[0], n_rows=100, k=3, ldx=3, row0=0, n_points=50, n_features=2, rowmean=P[1], out=P[2], ws=P[3],
             ws_bytes=BIG, stream=None),
        ('spr_rowstats_workspace', 'n_features'), ['spr_rowstats_x32']),
    'spr_feature_digit_hist_f64': (
        'X n_rows k ldx row0 n_points n_features prefix shift bits two out stream',
        dict(X=P[0], n_rows=100, k=3, ldx=3, row0=0, n_points=50, n_features=2, prefix=P[1], shift=0, bits=8, two=0,
             out=P[2], stream=None),
        None, ['spr_feature_digit_hist_x32']),
    'spr_qr_init_f64': (
        'Ur n_rows r ldu row0 nrm rec tau ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, nrm=P[1], rec=P[2], tau=P[3], ws=P[4], ws_bytes=BIG, stream=None),
        ('spr_qr_workspace_r', 'n_rows r'), ['spr_qr_init_u32']),
    'spr_qr_refresh_f64': (
        'Ur n_rows r ldu row0 Q piv j0 nq nrm rec tau ws ws_bytes stream',
        dict(Ur=P[0], n_rows=100, r=8, ldu=8, row0=0, Q=P[1], piv=P[2], j0=0, nq=1, nrm=P[3], rec=P[4], tau=P[5], ws=P[6],
             ws_bytes=BIG, stream=None),
        ('spr_qr_workspace_r', 'n_rows r'), ['spr_qr_refresh_u32']),
    # no feature layout unless scl is asked for, no cap on r (column groups), r = 0 is a valid call
    'spr_measure_csr_f64': (
        'indptr indices vals s Ur n_rows r ldu row0 rowmean scale n_points n_features Theta cnt scl stream',
        dict(indptr=P[0], indices=P[1], vals=P[2], s=5, Ur=P[3], n_rows=100, r=8, ldu=8, row0=0, rowmean=P[4], scale=None,
             n_points=0, n_features=0, Theta=P[5], cnt=P[6], scl=None, stream=None),
        None, ['spr_measure_csr_u32']),
}


def _other_cases():
    out = []
    for entry in ['spr_project_stream_f64'] + OTHER['spr_project_stream_f64'][3]:
        cap = _lib.SPR_MAX_R if entry.endswith('_x32') else _lib.SPR_MAX_R_STREAM     # f32 output: 128 columns per call
        out += [(entry, {'X': None}, INVALID, 'NULL'), (entry, {'ws': None}, INVALID, 'NULL'),
                (entry, {'k': 0}, INVALID, 'bad shape'), (entry, {'ldu': 7}, INVALID, 'bad r='),
                (entry, {'center': 3}, INVALID, 'centre mode'),
                (entry, {'row0': 1}, INVALID, 'bad feature layout'), (entry, {'row0': -1}, INVALID, 'bad feature layout'),
                (entry, {'r': cap + 1, 'ldu': cap + 1}, UNSUPPORTED, 'per call'),
                (entry, {'ws_bytes': 'one short'}, WORKSPACE, 'workspace'),
                (entry, {'ws': 24}, INVALID, '16-byte aligned'),
                # order: centre mode, layout, cap on r, workspace size, workspace alignment
                (entry, {'center': 3, 'row0': -1}, INVALID, 'centre mode'),
                (entry, {'row0': -1, 'r': cap + 1, 'ldu': cap + 1}, INVALID, 'bad feature layout'),
                (entry, {'r': cap + 1, 'ldu': cap + 1, 'ws_bytes': 0}, UNSUPPORTED, 'per call'),
                (entry, {'ws_bytes': 'one short', 'ws': 24}, WORKSPACE, 'workspace')]
    for fam in ('spr_feature_minmax_f64', 'spr_colsums_f64', 'spr_rowstats_f64', 'spr_feature_digit_hist_f64'):
        for entry in [fam] + OTHER[fam][3]:
            out += [(entry, {'X': None}, INVALID, 'NULL'), (entry, {'out': None}, INVALID, 'NULL'),
                    (entry, {'k': 0}, INVALID, 'bad shape'), (entry, {'ldx': 2}, INVALID, 'bad shape'),
                    (entry, {'row0': 1}, INVALID, 'bad shape'), (entry, {'row0': -1}, INVALID, 'bad shape'),
                    (entry, {'X': None, 'row0': -1}, INVALID, 'NULL')]
            if OTHER[fam][2]:
                out += [(entry, {'ws_bytes': 'one short'}, WORKSPACE, 'workspace too small'),
                        (entry, {'ws_bytes': 'one short', 'row0': -1}, INVALID, 'bad shape')]
    for entry in ('spr_feature_digit_hist_f64', 'spr_feature_digit_hist_x32'):
        out += [(entry, {'bits': 0}, INVALID, 'digit'), (entry, {'shift': 60}, INVALID, 'digit'),
                (entry, {'bits': 0, 'row0': -1}, INVALID, 'bad shape')]
    for fam in ('spr_qr_init_f64', 'spr_qr_refresh_f64'):
        for entry in [fam] + OTHER[fam][3]:
            big = {'r': _lib.SPR_MAX_R_WIDE + 1, 'ldu': _lib.SPR_MAX_R_WIDE + 1}
            out += [(entry, {'Ur': None}, INVALID, 'Ur is NULL'), (entry, {'ldu': 7}, INVALID, 'bad shape'),
                    (entry, {'n_rows': 0}, INVALID, 'bad shape'), (entry, big, UNSUPPORTED, 'not built'),
                    (entry, {'tau': None}, INVALID, 'NULL pointer'),
                    (entry, {'ws_bytes': 'one short'}, WORKSPACE, 'workspace too small'),
                    # order: the basis and its shape, the other pointers, the workspace
                    (entry, {'Ur': None, 'tau': None, 'ldu': 7}, INVALID, 'Ur is NULL'),
                    (entry, {'ldu': 7, 'tau': None}, INVALID, 'bad shape'),
                    (entry, dict(big, tau=None), UNSUPPORTED, 'not built'),
                    (entry, {'tau': None, 'ws_bytes': 0}, INVALID, 'NULL pointer')]
    for entry in ('spr_qr_refresh_f64', 'spr_qr_refresh_u32'):
        out += [(entry, {'nq': 0}, INVALID, 'bad j0='), (entry, {'j0': 8}, INVALID, 'bad j0='),
                (entry, {'nq': 0, 'ws_bytes': 0}, INVALID, 'bad j0=')]
    for entry in ['spr_measure_csr_f64'] + OTHER['spr_measure_csr_f64'][3]:
        no_basis = {'Ur': None, 'Theta': None, 'r': 0, 'ldu': 0}       # r = 0: neither is looked at (cnt / scl only)
        want_scl = {'scl': P[7], 'scale': P[8], 'n_points': 50, 'n_features': 2}
        out += [(entry, {name: None}, INVALID, 'NULL pointer') for name in ('indptr', 'indices', 'vals', 'rowmean', 'cnt', 'Ur', 'Theta')]
        out += [(entry, dict(no_basis, s=0), INVALID, 'bad shape s=0'),                  # ... so the next check is the one that fires
                (entry, dict(no_basis, indices=None), INVALID, 'NULL pointer'),
                (entry, {'Ur': None, 'Theta': None, 's': 0}, INVALID, 'NULL pointer'),   # r = 8: both are needed
                (entry, {'s': 0}, INVALID, 'bad shape s=0'), (entry, {'n_rows': 0}, INVALID, 'bad shape'),
                (entry, {'r': -1}, INVALID, 'bad shape'), (entry, {'ldu': 7}, INVALID, 'bad shape'),
                (entry, {'row0': -1}, INVALID, 'bad shape'),
                (entry, {'scl': P[7]}, INVALID, 'scl output needs the per-feature scale and layout'),
                (entry, dict(want_scl, scale=None), INVALID, 'scl output needs the per-feature scale and layout'),
                (entry, dict(want_scl, n_points=0), INVALID, 'scl output needs the per-feature scale and layout'),
                (entry, dict(want_scl, n_features=0), INVALID, 'scl output needs the per-feature scale and layout'),
                # order: the pointers, the shape, what scl needs
                (entry, {'vals': None, 's': 0, 'scl': P[7]}, INVALID, 'NULL pointer'),
                (entry, {'row0': -1, 'scl': P[7]}, INVALID, 'bad shape')]
    return out


# the cap on r of each family that has one: (largest r taken, status of the refusal)
R_CAP = {
    'spr_bound_sweep_f64': (_lib.SPR_MAX_R_WIDE, UNSUPPORTED),
    'spr_bound_sweep_batch_f64': (_lib.SPR_MAX_R_WIDE, UNSUPPORTED),
    'spr_encode_f64': (_lib.SPR_MAX_R_WIDE, UNSUPPORTED),
    'spr_field_error_f64': (_lib.SPR_MAX_R_WIDE, UNSUPPORTED),
    'spr_gappy_normal_f64': (_lib.SPR_MAX_R, INVALID),
    'spr_gappy_fill_f64': (_lib.SPR_MAX_R, UNSUPPORTED),
    'spr_field_std_diag_f64': (_lib.SPR_MAX_R_WIDE, UNSUPPORTED),
    'spr_field_std_factor_f64': (_lib.SPR_MAX_R, INVALID),
}


def _entries(family):
    return [family] + FAMILIES[family][3]


def _cases():
    """(entry, changed arguments, status, text fragment)"""
    out = []
    for fam, (_, good, wsfn, _) in FAMILIES.items():
        first_ptr = 'X' if fam == 'spr_project_f64' else 'Ur'
        last_ptr = next(n for n in ('W', 'A', 'S', 'G', 'nobs') if n in good)
        for entry in _entries(fam):
            out.append((entry, {first_ptr: None}, INVALID, 'NULL'))
            out.append((entry, {last_ptr: None}, INVALID, 'NULL'))
            out.append((entry, {'ldu': good['r'] - 1}, INVALID, 'bad '))                    # ldu < r
            out.append((entry, {'k': 0}, INVALID, 'bad shape'))
            out.append((entry, {'row0': 1}, INVALID, 'bad feature layout'))                 # one row past the last feature
            out.append((entry, {'row0': -1}, INVALID, 'bad feature layout'))
            out.append((entry, {'n_features': 0}, INVALID, 'bad feature layout'))
            # two defects at once: the pointers are looked at before the shape, the shape before the layout
            out.append((entry, {first_ptr: None, 'k': 0}, INVALID, 'NULL'))
            out.append((entry, {'k': 0, 'row0': -1}, INVALID, 'bad shape'))
            if fam in R_CAP:
                cap, status = R_CAP[fam]
                over = {'r': cap + 1, 'ldu': cap + 1}
                out.append((entry, over, status, 'exceeds'))
                # ... the layout before the cap on r, and the cap before the size of the workspace
                out.append((entry, dict(over, row0=-1), INVALID, 'bad feature layout'))
                if wsfn:
                    out.append((entry, dict(over, ws_bytes=0), status, 'exceeds'))
            if wsfn:
                out.append((entry, {'ws_bytes': 'one short'}, INVALID, 'workspace of'))
                out.append((entry, {'ws_bytes': 'one short', 'row0': -1}, INVALID, 'bad feature layout'))
    # checks only some families have
    for entry in _entries('spr_bound_sweep_f64') + _entries('spr_bound_sweep_batch_f64'):
        out.append((entry, {'tol': -1.0}, INVALID, 'tol'))
        out.append((entry, {'tol': -1.0, 'row0': -1}, INVALID, 'bad feature layout'))       # layout, then tol, then r
        out.append((entry, {'tol': -1.0, 'r': 1025, 'ldu': 1025}, INVALID, 'tol'))
    for entry in _entries('spr_field_std_factor_f64'):
        out.append((entry, {'q': 0}, INVALID, 'outside'))
        out.append((entry, {'q': 9}, INVALID, 'outside'))                                   # q > r
        out.append((entry, {'q': 0, 'r': 129, 'ldu': 129}, INVALID, 'exceeds'))             # r before q
    for entry in _entries('spr_project_f64'):
        out.append((entry, {'r': 129, 'ldu': 129}, UNSUPPORTED, 'not built'))
        out.append((entry, {'k': 257, 'ldx': 257}, UNSUPPORTED, 'not built'))
        out.append((entry, {'r': 129, 'ldu': 129, 'row0': -1}, INVALID, 'bad feature layout'))
    return out


def _id(case):
    entry, change, _, _ = case
    return entry[4:] + '-' + '+'.join(f'{k}={v}'.replace(' ', '_') for k, v in change.items())


@pytest.mark.parametrize('case', _cases() + _other_cases(), ids=_id)
def test_refusal(case):
    entry, change, status, fragment = case
    lib = _lib.load()
    table = dict(FAMILIES, **OTHER)
    fam = next(f for f in table if entry == f or entry in table[f][3])
    names, good, wsfn, _ = table[fam]
    args = dict(good, **change)
    args['x32'] = int('_x32' in entry)     # spr_project_stream_workspace asks for the storage type of X
    if args.get('ws_bytes') == 'one short':
        need = getattr(lib, wsfn[0])(*[args[n] for n in wsfn[1].split()])
        assert need > 1
        args['ws_bytes'] = need - 1
    rc = getattr(lib, entry)(*[args[n] for n in names.split()])
    text = lib.spr_last_error().decode()
    assert rc == status, (rc, text)
    assert text.startswith(entry + ': '), text
    assert fragment in text, text


def test_workspace_functions_refuse_empty_shapes():
    lib = _lib.load()
    assert lib.spr_bound_sweep_workspace(0, 2) == 0 and lib.spr_bound_sweep_workspace(3, 0) == 0
    assert lib.spr_encode_workspace(0, 3, 2) == 0 and lib.spr_field_error_workspace(0, 2) == 0
    assert lib.spr_gappy_normal_workspace(_lib.SPR_MAX_R + 1, 3, 2) == 0
    assert lib.spr_bound_sweep_batch_workspace(3, 2) == lib.spr_bound_sweep_workspace(3, 2) > 0

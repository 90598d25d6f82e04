#!/usr/bin/env python3
"""Record what the UNMODIFIED reference camera (openmeasure.utils.camera) hands to its mesh, as a data fixture.

    python tools/make_camera_record.py [--reference DIR] [--out tests/golden/camera_segments.json]

The reference's utils.py is loaded from DIR (the directory that holds the ``openmeasure`` package; default: the
environment variable OPENMEASURE_REFERENCE, else the place oracle/make_golden.py reads it from) with an in-memory stand-in
for the ``pyvista`` module, which is not needed for the geometry.  ``camera.project`` then runs over a stand-in mesh whose
``find_cells_intersecting_line`` records its two arguments and returns no cell.  For the random models NumPy's
``default_rng`` is wrapped for the duration of the call, so that the uniform numbers the reference draws are recorded in the
order it draws them.  Nothing of the reference's text is written anywhere: the output holds attributes, the extrinsic
matrix, the sensor coordinates, the draws and the recorded end points of a 4 x 3-pixel camera with N_rand = 2 for two
parameter sets (the second with m > 0, the only one the thin-lens model accepts)."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAND = 2
SENSOR_PX = (4, 3)
PARAMETER_SETS = [
    # the notebook's orientation and lens (f = d_sensor = 1: m = 0, focus at infinity)
    dict(name='notebook', p_cam=[1.0, 0.0, 0.3, 1.0], theta=[-np.pi / 2, 0.0, -np.pi / 2], f_length=1.0, n_aper=1.0,
         d_sensor=1.0, px_size=0.1),
    # a tilted camera focused at a finite distance (m = 0.2)
    dict(name='focused', p_cam=[0.7, -0.4, 0.55, 1.0], theta=[-1.3, 0.21, -1.75], f_length=0.05, n_aper=2.8, d_sensor=0.06,
         px_size=0.004),
]


def load_reference_utils(ref_dir):
    path = os.path.join(ref_dir, 'openmeasure', 'utils.py')
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    had = sys.modules.get('pyvista')
    sys.modules['pyvista'] = types.ModuleType('pyvista')      # the module is imported, never used, by what runs here
    try:
        spec = importlib.util.spec_from_file_location('_reference_openmeasure_utils', path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if had is None:
            del sys.modules['pyvista']
        else:
            sys.modules['pyvista'] = had
    return mod


class RecordingMesh:
    n_cells = 1

    def __init__(self):
        self.lines = []

    def find_cells_intersecting_line(self, a, b):
        self.lines.append((np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)))
        return []


class RecordingRng:
    """what the reference uses of a Generator: random(size=...)"""

    def __init__(self, inner, log):
        self.inner, self.log = inner, log

    def random(self, size=None):
        u = self.inner.random(size=size)
        self.log.append(np.array(u, dtype=np.float64))
        return u


def record_model(cam, type_rec, seed):
    """-> dict(a, b[, jitter][, lens]) with the layout of openmeasure_amd.utils.camera.segments"""
    mesh, log = RecordingMesh(), []
    inner = np.random.Generator(np.random.PCG64(seed))
    real = np.random.default_rng
    np.random.default_rng = lambda *args, **kw: RecordingRng(inner, log)
    try:
        cam.project(mesh, type_rec=type_rec, N_rand=N_RAND)
    finally:
        np.random.default_rng = real
    n_pix = cam.n_pixels
    n_ray = 1 if type_rec == 'parallel' else N_RAND
    assert len(mesh.lines) == n_pix * n_ray, (type_rec, len(mesh.lines))
    out = dict(a=np.stack([l[0] for l in mesh.lines]).reshape(n_pix, n_ray, 3).tolist(),
               b=np.stack([l[1] for l in mesh.lines]).reshape(n_pix, n_ray, 3).tolist())
    if type_rec == 'parallel':
        assert not log
        return out
    if type_rec == 'thin_lens':                               # two draws of n_pix * N_rand lens numbers come first
        lens_r, lens_t = log[0], log[1]
        assert lens_r.shape == lens_t.shape == (n_pix * N_RAND,)
        out['lens'] = np.stack([lens_r[:n_pix], lens_t[:n_pix]], axis=1).tolist()
        log = log[2:]
    assert len(log) == 2 * n_pix and all(u.shape == (N_RAND,) for u in log)   # per pixel: N_rand for x, N_rand for y
    out['jitter'] = np.stack([np.stack([log[2 * i], log[2 * i + 1]], axis=1) for i in range(n_pix)]).tolist()
    return out


def make_record(ref_dir):
    ref = load_reference_utils(ref_dir)
    sets = []
    for k, p in enumerate(PARAMETER_SETS):
        cam = ref.camera(np.array(p['p_cam']), np.array(p['theta']), p['f_length'], p['n_aper'], p['d_sensor'],
                         np.array(SENSOR_PX), p['px_size'])
        rec = dict(parameters={key: (val if not isinstance(val, list) else [float(v) for v in val]) for key, val in p.items()},
                   sensor_size_px=list(SENSOR_PX), N_rand=N_RAND,
                   attributes=dict(n_pixels=int(cam.n_pixels), sensor_size_m=np.asarray(cam.sensor_size_m, float).tolist(),
                                   d=float(cam.d), m=float(cam.m), d_object=float(cam.d_object)),
                   E=cam._extr_matrix().tolist(), sensor_coordinates=cam._sensor_coordinates().tolist(), models={})
        for j, type_rec in enumerate(('parallel', 'pinhole', 'thin_lens')):
            if type_rec == 'thin_lens' and cam.m == 0:
                rec['models'][type_rec] = None                # the reference raises ValueError: focus at infinity
                continue
            rec['models'][type_rec] = record_model(cam, type_rec, seed=1000 + 10 * k + j)
        sets.append(rec)
    return dict(what='end points handed to find_cells_intersecting_line by the reference camera; see tools/make_camera_record.py',
                sets=sets)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', default=os.environ.get('OPENMEASURE_REFERENCE', '/root/reference/src'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'camera_segments.json'))
    args = ap.parse_args()
    with open(args.out, 'w') as f:
        json.dump(make_record(args.reference), f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Record what the UNMODIFIED reference returns or raises on the inputs of tests/test_reference_differential.py, into
tests/golden/reference_outcomes.json (values, shapes, dtypes, exception types and texts, method signatures).

Runs only where the reference is installed (it is imported as make_golden.py imports it, with the same one-function cvxpy
stand-in); the test itself reads nothing but the record.  The inputs and the way each outcome is taken are the test module's
own functions, so the record and the test cannot drift apart.

Usage:  python oracle/make_reference_record.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.make_golden import _import_reference  # noqa: E402
from tests import test_reference_differential as t  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'reference_outcomes.json')


def main():
    sps = _import_reference()
    ns = types.SimpleNamespace(SPR=sps.SPR, ROM=sps.ROM)
    rec = dict(
        note='outcomes of the unmodified reference on the inputs of tests/test_reference_differential.py '
             '(written by oracle/make_reference_record.py)',
        fit={t.fit_key(*c): t.record_fit(ns, *c) for c in t.FIT_CASES},
        fit_errors={repr(sorted(kw.items())): t.record_fit_error(ns, kw) for kw, _ in t.FIT_ERRORS},
        axis_cnt={str(a): t.record_axis_cnt(ns, a) for a in t.AXIS_CNTS},
        misshaped_sampling=t.record_misshaped_sampling(ns),
        attributes=t.attribute_record(t.record_attributes(ns)),
        signatures=t.record_signatures(sps),
        cases=t._differential_cases(ns),
    )
    with open(OUT, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB, {len(rec["cases"])} host-logic cases')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""PI rows of the cases of tests/test_gpu_pi_partial_slots.py as one array, for a byte comparison of two library builds:

    TPHIP_LIB=<libA.so> python tools/debug/pi_rows_dump.py a.npy
    TPHIP_LIB=<libB.so> python tools/debug/pi_rows_dump.py b.npy
    cmp a.npy b.npy

The cases are the test module's own (CASE_KEYS / make_case).  Every case's locus goes behind 0..3 filler chunks, as in
the test; all rows (fillers included) are written, padded to the widest table."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(path):
    import test_gpu_pi_partial_slots as t
    from tapir_amd import engine
    setup = t.make_setup()
    pin = setup["pin"]
    fr, fn = setup["filler"]
    rows = []
    for key in t.CASE_KEYS:
        c = t.make_case(setup, key)
        T = int(pin["T"]) if c["T"] is None else c["T"]
        for k in range(4):
            plan = t._plan(engine, pin, [t.CHUNK] * k + [len(c["rates"])], T, [0, T - 1], c["intervals"])
            try:
                rows.extend(plan.pi_tables(np.concatenate([fr] * k + [c["rates"]]), np.concatenate([fn] * k + [c["nres"]])))
            finally:
                plan.close()
    width = max(len(r) for r in rows)
    out = np.zeros((len(rows), width))
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    np.save(path, out)
    print("%d cases, %d rows, widest %d -> %s" % (len(t.CASE_KEYS), len(rows), width, path))


if __name__ == "__main__":
    main(sys.argv[1])

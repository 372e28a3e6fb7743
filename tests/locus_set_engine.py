"""The CPU stand-in engine (tests/exact_quartet_engine.py, so every quartet flag and --exact-quartets work) with the locus-set
calls of tapir_amd/engine.py, answered by tests/locus_set_reference.py.  "Device" buffers are numpy arrays; a `_dev` call fills
the array it is given.  Test helper."""
import numpy as np

import exact_quartet_engine
import exact_quartet_reference as er
import locus_set_reference as lr

CALLS = []


def __getattr__(name):
    return getattr(exact_quartet_engine, name)


def _check_order(order, nloci):
    order = np.asarray(order)
    assert order.ndim == 2 and 1 <= order.shape[0] <= 256 and 1 <= order.shape[1] <= nloci, order.shape
    assert order.min() >= 0 and order.max() < nloci
    for row in order:
        assert len(set(row.tolist())) == len(row), "a locus index is repeated within a quartet"
    return order


def locus_set_rows(locus_rows, order, device=0):
    locus_rows = np.asarray(locus_rows, np.float64)
    order = _check_order(order, locus_rows.shape[0])
    assert locus_rows.ndim == 3 and locus_rows.shape[2] in (8, 13) and locus_rows.shape[1] == order.shape[0]
    CALLS.append(("locus_set_rows", locus_rows.shape, order.shape))
    return lr.normal_rows(locus_rows, order)


class Plan(exact_quartet_engine.Plan):
    def locus_set_exact_workspace_bytes(self, n_q, n_k, window_cap=128, n_head=0):
        assert 1 <= n_q <= 256 and 1 <= n_k <= self.nloci and 0 <= n_head <= n_k and window_cap in (16, 32, 64, 128, 256, 512)
        return 256

    def locus_set_exact(self, y, x1, x2, order, window_cap=128, tail_tolerance=0.0, n_head=0):
        y, x1, x2 = (np.asarray(v, np.float64) for v in (y, x1, x2))
        order = _check_order(order, self.nloci)
        assert y.shape == x1.shape == x2.shape == (order.shape[0], self.ncols) and 0 <= n_head <= order.shape[1]
        CALLS.append(("locus_set_exact", order.shape, window_cap, n_head, self.nloci))
        return np.stack([lr.exact_rows((y[q], x1[q], x2[q]), self.off, order[q], window_cap, tail_tolerance or er.DEFAULT_TAIL, n_head)
                         for q in range(order.shape[0])])

    def locus_set_exact_dev(self, d_y, d_x1, d_x2, order, d_rows, d_ws, window_cap=128, tail_tolerance=0.0, n_head=0, stream=0):
        d_rows[...] = self.locus_set_exact(d_y, d_x1, d_x2, order, window_cap, tail_tolerance, n_head)

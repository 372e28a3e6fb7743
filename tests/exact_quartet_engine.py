"""The CPU stand-in engine (tests/unequal_quartet_engine.py, so every quartet flag works) with engine.Plan's exact-quartet calls
and the device-buffer helpers pipeline.exact_quartet_tables uses, answered by tests/exact_quartet_reference.py.  "Device"
buffers are numpy arrays; a `_dev` call fills the array it is given.  Test helper."""
import numpy as np

import exact_quartet_reference as er
import unequal_quartet_engine

CALLS = []


def __getattr__(name):
    return getattr(unequal_quartet_engine, name)


def device_empty(shape, device, dtype=np.float64):
    return np.full(tuple(shape), 0, dtype=dtype)


def device_array(a, device):
    return np.array(a, copy=True)


def host_array(t):
    return np.array(t, copy=True)


def device_stream(device):
    return 0


class Plan(unequal_quartet_engine.Plan):
    def quartet_sites_dev(self, d_rates, d_nres, quartets, d_sites, stream=0):
        d_sites[...] = self.quartet_sites(d_rates, d_nres, quartets)

    def unequal_quartet_sites_dev(self, d_rates, d_nres, quartets, d_sites, stream=0):
        d_sites[...] = self.unequal_quartet_sites(d_rates, d_nres, quartets)

    def quartet_exact_workspace_bytes(self, n_q, window_cap=128):
        assert 1 <= n_q <= 256 and window_cap in (16, 32, 64, 128, 256, 512)
        return 256

    def quartet_exact(self, y, x1, x2, window_cap=128, tail_tolerance=0.0):
        y, x1, x2 = (np.asarray(v, np.float64) for v in (y, x1, x2))
        assert y.shape == x1.shape == x2.shape and y.shape[1] == self.ncols and 1 <= y.shape[0] <= 256
        CALLS.append(("exact", y.shape[0], window_cap, self.nloci))
        rows = np.zeros((self.nloci, y.shape[0], 6))
        for l in range(self.nloci):
            sl = slice(self.off[l], self.off[l + 1])
            for q in range(y.shape[0]):
                rows[l, q] = er.resolution(y[q, sl], x1[q, sl], x2[q, sl], window_cap, tail_tolerance or er.DEFAULT_TAIL)
        return rows

    def quartet_exact_dev(self, d_y, d_x1, d_x2, n_q, d_rows, d_ws, window_cap=128, tail_tolerance=0.0, stream=0):
        assert d_y.shape[0] == n_q
        d_rows[...] = self.quartet_exact(d_y, d_x1, d_x2, window_cap, tail_tolerance)

"""The CPU stand-in engine (tests/oracle_engine.py) with engine.Plan's site-bootstrap call, answered by
tests/bootstrap_reference.py: the reference's counts, per-site PI values in fp64 and numpy's summary.  Test helper."""
import numpy as np

import bootstrap_reference as bsr
import hp_reference as hp
import oracle_engine

CALLS = []


def __getattr__(name):
    return getattr(oracle_engine, name)


class Plan(oracle_engine.Plan):
    @property
    def bootstrap_width(self):
        return self.T + len(self.intervals)

    def pi_bootstrap(self, rates, nres=None, replicates=200, seed=1, level=0.95, locus_ids=None, return_rows=False):
        fin = hp.finalize_rates(rates, self.round_decimals, self.correction, nres, self.threshold)
        ids = np.arange(self.nloci) if locus_ids is None else np.asarray(locus_ids, np.int64)
        assert ids.shape == (self.nloci,) and 2 <= replicates <= 4096 and 0.0 < level < 1.0
        CALLS.append(("bootstrap", int(replicates), int(seed), float(level), ids.tolist()))
        Wb = self.bootstrap_width
        summary, rows = np.zeros((self.nloci, 4, Wb)), np.zeros((self.nloci, replicates, Wb))
        t = np.arange(self.T, dtype=np.float64)
        for l in range(self.nloci):
            r = fin[self.off[l]:self.off[l + 1]]
            live = np.isfinite(r) & (r != 0.0)
            vals = np.zeros((r.size, Wb))
            rr = r[live][:, None]
            vals[live, :self.T] = 16.0 * rr * rr * t[None, :] * np.exp(-4.0 * rr * t[None, :])
            vals[:, self.T:] = bsr.site_integrals(r, self.intervals.tolist(), exact=self.integ_mode == 1)
            cnt = bsr.counts(seed, int(ids[l]), r.size, 0, replicates)
            rows[l] = cnt.astype(np.float64) @ vals
            summary[l] = bsr.summarize(rows[l], level)
        return (summary, rows) if return_rows else summary

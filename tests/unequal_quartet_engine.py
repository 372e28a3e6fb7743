"""The CPU stand-in engine (tests/quartet_engine.py, so --quartets works beside the new flags) with engine.Plan's
unequal-quartet calls, answered by the fp64 restatement of tests/unequal_quartet_reference.py.  Test helper."""
import numpy as np

import hp_reference as hp
import quartet_engine
import unequal_quartet_reference as ur

CALLS = []


def __getattr__(name):
    return getattr(quartet_engine, name)


class Plan(quartet_engine.Plan):
    @staticmethod
    def _unequal_quartets(quartets):
        quartets = np.asarray(quartets, np.float64).reshape(-1, 5)
        assert 1 <= len(quartets) <= 256 and np.all(np.isfinite(quartets)) and np.all(quartets[:, :4] >= 0) and np.all(quartets[:, 4] > 0)
        return quartets

    def unequal_quartet_workspace_bytes(self, quartets):
        return 256

    def unequal_quartet_sites(self, rates, nres, quartets):
        quartets = self._unequal_quartets(quartets)
        fin = hp.finalize_rates(rates, self.round_decimals, self.correction, nres, self.threshold)
        out = np.zeros((3, len(quartets), self.ncols))
        for l in range(self.nloci):
            sl = slice(self.off[l], self.off[l + 1])
            for q, row in enumerate(quartets.tolist()):
                out[0, q, sl], out[1, q, sl], out[2, q, sl] = ur.site_values(self.model, self.pi[l], self.exch[l], fin[sl], row[:4], row[4])
        return out

    def unequal_quartet_tables(self, rates, nres, quartets):
        quartets = self._unequal_quartets(quartets)
        CALLS.append(("unequal_quartets", self.model, quartets.tolist(), self.nloci))
        sites = self.unequal_quartet_sites(rates, nres, quartets)
        rows = np.zeros((self.nloci, len(quartets), 13))
        for l in range(self.nloci):
            sl = slice(self.off[l], self.off[l + 1])
            for q in range(len(quartets)):
                rows[l, q, :9] = ur.locus_sums(sites[0, q, sl], sites[1, q, sl], sites[2, q, sl])
                rows[l, q, 9:] = ur.probabilities(rows[l, q, :9])
        return rows

"""The CPU stand-in engine (tests/oracle_engine.py) with engine.Plan's quartet calls, answered by the fp64 restatement of
tests/quartet_reference.py.  Test helper."""
import numpy as np

import hp_reference as hp
import oracle_engine
import quartet_reference as qr

CALLS = []


def __getattr__(name):
    return getattr(oracle_engine, name)


class Plan(oracle_engine.Plan):
    def __init__(self, ntaxa, parent, branch_len, leaf_taxon, locus_offsets, pi, exch, *args, model="gtr", **kw):
        assert model in ("gtr", "f81") and (exch is None) == (model == "f81")
        L = len(locus_offsets) - 1
        super().__init__(ntaxa, parent, branch_len, leaf_taxon, locus_offsets, pi, np.ones((L, 6)) if exch is None else exch, *args, **kw)
        self.model = model

    def quartet_sites(self, rates, nres, quartets):
        quartets = np.asarray(quartets, np.float64).reshape(-1, 2)
        assert 1 <= len(quartets) <= 256 and np.all(quartets[:, 0] >= 0) and np.all(quartets[:, 1] > 0)
        fin = hp.finalize_rates(rates, self.round_decimals, self.correction, nres, self.threshold)
        out = np.zeros((2, len(quartets), self.ncols))
        for l in range(self.nloci):
            sl = slice(self.off[l], self.off[l + 1])
            for q, (tip, internode) in enumerate(quartets):
                out[0, q, sl], out[1, q, sl] = qr.site_values(self.model, self.pi[l], self.exch[l], fin[sl], tip, internode)
        return out

    def quartet_tables(self, rates, nres, quartets):
        quartets = np.asarray(quartets, np.float64).reshape(-1, 2)
        CALLS.append(("quartets", self.model, quartets.tolist(), self.nloci))
        sites = self.quartet_sites(rates, nres, quartets)
        rows = np.zeros((self.nloci, len(quartets), 8))
        for l in range(self.nloci):
            sl = slice(self.off[l], self.off[l + 1])
            for q in range(len(quartets)):
                rows[l, q, :5] = qr.locus_sums(sites[0, q, sl], sites[1, q, sl])
                rows[l, q, 5:] = qr.probabilities(rows[l, q, :5])
        return rows

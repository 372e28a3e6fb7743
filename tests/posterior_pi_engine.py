"""The CPU stand-in engine (tests/eb_engine.py) with engine.Plan's posterior-PI calls, answered by tests/eb_reference.py (the
category posterior) and tests/posterior_pi_reference.py (category rows, analytic moments, the mirror of the draws) with
numpy's summary.  Test helper."""
import math

import numpy as np

import bootstrap_reference as bsr
import eb_engine
import eb_reference as ebr
import posterior_pi_reference as ppr

CALLS = []


def __getattr__(name):
    return getattr(eb_engine, name)


class Plan(eb_engine.Plan):
    @property
    def bootstrap_width(self):
        return self.T + len(self.intervals)

    def models(self):
        """(lam, U, Ui, kappa) of engine.Plan.models: only kappa is answered."""
        return None, None, None, np.array([ebr.kappa(self.pi[l], self.exch[l]) for l in range(self.nloci)])

    def eb_posterior_table(self, states, cat_rate, cat_weight, scale, use_patterns=True):
        cat_rate, cat_weight = np.asarray(cat_rate, np.float64), np.asarray(cat_weight, np.float64)
        CALLS.append(("table", cat_rate.shape[1]))
        out = self.eb_posterior(states, cat_rate, cat_weight, scale, use_patterns)
        out["post"] = np.zeros((cat_rate.shape[1], self.ncols))
        for l, loc in self._loci(states):
            out["post"][:, self.off[l]:self.off[l + 1]] = loc.posterior_of(math.log(scale[l]), cat_rate[l], cat_weight[l])["weights"]
        return out

    def posterior_pi_workspace_bytes(self, ncat, replicates, seed=1, level=0.95):
        return 1, 1

    def posterior_pi(self, post, nres, scale, cat_rate, replicates=200, seed=1, level=0.95, locus_ids=None, return_rows=False,
                     return_counts=False):
        post, cat_rate = np.asarray(post, np.float64), np.asarray(cat_rate, np.float64)
        K, B = cat_rate.shape[1], int(replicates)
        assert post.shape == (K, self.ncols) and 2 <= B <= 4096 and 0.0 < level < 1.0 and 2 <= K <= 16
        ids = np.arange(self.nloci) if locus_ids is None else np.asarray(locus_ids, np.int64)
        CALLS.append(("posterior_pi", B, int(seed), float(level), ids.tolist()))
        Wb = self.bootstrap_width
        out = dict(analytic=np.zeros((self.nloci, 2, Wb)), expected_counts=np.zeros((self.nloci, K)),
                   summary=np.zeros((self.nloci, 4, Wb)), rows=np.zeros((self.nloci, B, Wb)),
                   counts=np.zeros((self.nloci, B, K), np.int32))
        kappa = self.models()[3]
        for l in range(self.nloci):
            sl = slice(self.off[l], self.off[l + 1])
            live = None if nres is None else np.asarray(nres)[sl] >= self.threshold
            r = ppr.category_rates(kappa[l], scale[l], cat_rate[l], self.round_decimals, self.correction)
            P = ppr.category_rows(r, self.T, self.intervals.tolist(), exact=self.integ_mode == 1)
            nk, mean, sd = ppr.analytic(post[:, sl], live, P)
            out["expected_counts"][l], out["analytic"][l, 0], out["analytic"][l, 1] = nk, mean, sd
            out["counts"][l] = ppr.counts(post[:, sl], live, seed, int(ids[l]), B)
            out["rows"][l] = out["counts"][l].astype(np.float64) @ P
            out["summary"][l] = bsr.summarize(out["rows"][l], level)
        if not return_rows:
            del out["rows"]
        if not return_counts:
            del out["counts"]
        return out

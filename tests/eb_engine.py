"""The CPU stand-in engine (tests/site_model_engine.py) with the two empirical-Bayes calls of engine.Plan, answered by
tests/eb_reference.py: eb_fit_scale by the reference's bounded scalar search, eb_posterior by its posterior.  Test helper."""
import math

import numpy as np

import eb_reference as ebr
import site_model_engine

CALLS = []


def __getattr__(name):
    return getattr(site_model_engine, name)


class Plan(site_model_engine.Plan):
    def _loci(self, states):
        states = np.asarray(states, np.uint8)
        for l in range(self.nloci):
            yield l, ebr.Locus(states[:, self.off[l]:self.off[l + 1]], self.parent, self.blen, self.leaf, self.pi[l], self.exch[l])

    def eb_start_scale(self, states):
        from tapir_amd import eb
        return eb.start_scales(states, self.off, self.parent, self.blen, self.leaf)

    def eb_fit_scale(self, states, cat_rate, cat_weight, scale, use_patterns=True, maxit_scale=0, tol_scale=0.0):
        cat_rate, cat_weight = np.asarray(cat_rate, np.float64), np.asarray(cat_weight, np.float64)
        assert cat_rate.shape == cat_weight.shape and cat_rate.shape[0] == self.nloci and np.all(np.asarray(scale) > 0)
        CALLS.append(("fit", cat_rate.shape[1]))
        out = dict(scale=np.empty(self.nloci), locus_lnl=np.empty(self.nloci), curvature=np.full(self.nloci, np.nan),
                   iters=np.ones(self.nloci, np.int32))
        for l, loc in self._loci(states):
            u, val = loc.fit_scale_of(cat_rate[l], cat_weight[l], grid=49)
            out["scale"][l], out["locus_lnl"][l] = math.exp(u), val
        return out

    def eb_posterior(self, states, cat_rate, cat_weight, scale, use_patterns=True):
        cat_rate, cat_weight = np.asarray(cat_rate, np.float64), np.asarray(cat_weight, np.float64)
        CALLS.append(("posterior", cat_rate.shape[1]))
        out = dict(rate=np.empty(self.ncols), sd=np.empty(self.ncols), lnl=np.empty(self.ncols), nres=np.empty(self.ncols, np.int32))
        states = np.asarray(states, np.uint8)
        for l, loc in self._loci(states):
            sl = slice(self.off[l], self.off[l + 1])
            p = loc.posterior_of(math.log(scale[l]), cat_rate[l], cat_weight[l])
            out["rate"][sl], out["sd"][sl], out["lnl"][sl] = p["rate"], p["sd"], p["ll"]
            out["nres"][sl] = ebr.orc.informative_counts(states[:, sl])
        return out

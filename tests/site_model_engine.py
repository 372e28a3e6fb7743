"""The CPU stand-in engine (tests/oracle_engine.py) with the `model` argument of engine.Plan: model="f81" is the oracle
with exchangeabilities of 1 (exch must be None, as tphip_plan_desc requires).  Records the models of the plans it makes;
the stage-1 entry point raises, so a run that reaches stage 1 fails."""
import numpy as np

import oracle_engine

PLANS = []


def __getattr__(name):   # everything else (state_histogram, compress_columns, ...) is oracle_engine's
    return getattr(oracle_engine, name)


class Plan(oracle_engine.Plan):
    def __init__(self, ntaxa, parent, branch_len, leaf_taxon, locus_offsets, pi, exch, *args, model="gtr", **kw):
        assert model in ("gtr", "f81")
        if model == "f81":
            assert exch is None, "an F81 plan takes no exchangeabilities"
            exch = np.ones((len(locus_offsets) - 1, 6))
        super().__init__(ntaxa, parent, branch_len, leaf_taxon, locus_offsets, pi, exch, *args, **kw)
        self.model = model
        PLANS.append(model)

    def locus_loglik(self, *args, **kw):
        raise AssertionError("stage 1 ran under a fixed site model")

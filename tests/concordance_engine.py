"""The CPU stand-in engine (tests/locus_set_engine.py, so every other flag of the command line works) with the two concordance
calls of tapir_amd/engine.py, answered by tests/concordance_reference.py.  It refuses what the library refuses.  Test helper."""
import numpy as np

import concordance_reference as cr
import locus_set_engine

CALLS = []


def __getattr__(name):
    return getattr(locus_set_engine, name)


def concordance_counts(states, locus_offsets, group_offsets, group_taxa, ncols_total=None, device=0):
    states = np.asarray(states, np.uint8)
    off = np.asarray(locus_offsets, np.int64)
    ncols = states.shape[1] if ncols_total is None else int(ncols_total)
    sets = cr.split_sets(group_offsets, group_taxa)
    assert states.ndim == 2 and states.shape[0] >= 4 and len(sets) >= 1 and ncols <= states.shape[1]
    assert off[0] >= 0 and off[-1] <= ncols and np.all(np.diff(off) >= 0)
    for groups in sets:
        named = [t for g in groups for t in g]
        assert all(len(g) >= 1 for g in groups) and len(set(named)) == len(named), "an empty group or a taxon listed twice"
        assert min(named) >= 0 and max(named) < states.shape[0]
    CALLS.append(("concordance_counts", states.shape, len(off) - 1, len(sets)))
    return cr.counts_np(states, off, group_offsets, group_taxa)


def concordance_rows(counts, node_sets, device=0):
    counts = np.asarray(counts, np.uint64)
    nodes = np.asarray(node_sets, np.int64)
    assert counts.ndim == 3 and counts.shape[2] == 3 and nodes[0] >= 0 and nodes[-1] <= counts.shape[1] and np.all(np.diff(nodes) >= 2)
    assert int(counts.max(initial=0)) < 2 ** 53
    CALLS.append(("concordance_rows", counts.shape, len(nodes) - 1))
    return cr.rows(counts.tolist(), nodes)

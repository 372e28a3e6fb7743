#!/usr/bin/env python3
"""Sweep of the later shares' geometry with the CPU replay (tools/share_replay.py; no GPU needed): rounds and makespan of
site_rate_kernel's hand-out by predicted work for later shares of equal column counts against whole lane-fills x 1/2/3/4 and
tapers, at reserves 0.10-0.35.  profiles/r17_tail_share_sweep.txt is its output.

  python tools/debug/tail_share_sweep.py [--loci 2 --cols 20000 --taxa 64 --seed 5 --waves 16 --grid-mult 3] [--cache evals.npy]

The default batch has the share geometry of bench.py's C3 at 16 waves: first-round shares of about 1 700 columns inside long
loci.  --cache keeps the oracle's evaluation counts of the batch (one call per column) between runs.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import share_replay as rp  # noqa: E402

GEOMETRIES = ["0", "1,1,1", "2,2,2", "3,3,3", "4,4,4", "4,2,1,0.5,0.25", "6,3,1,0.5,0.25", "8,4,2,0.5,0.25", "4,3,2,0.5,0.25", "6,3,2,0.5,0.25",
              "5,3,2,0.4,0.3", "4,2,1,0.25,0.25"]
ALIGNED = ["8,4,2,0.5,0.25+loci", "5,3,2,0.4,0.3+loci", "2,2,2+loci"]
RESERVES = [0.10, 0.15, 0.20, 0.25, 0.30, 0.35]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=2)
    ap.add_argument("--cols", type=int, default=20000)
    ap.add_argument("--taxa", type=int, default=64)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--waves", type=int, default=16)
    ap.add_argument("--grid-mult", type=int, default=3)
    ap.add_argument("--cache", default=None)
    a = ap.parse_args()
    from tapir_amd import synth
    d = synth.simulate(a.loci, a.cols, a.taxa, a.seed)
    pin = synth.plan_inputs(d["root"], d["names"])
    st, off = d["states"].numpy(), d["locus_offsets"]
    optimised, slow = rp.classify(st, pin["parent"], pin["leaf"])
    if a.cache and os.path.exists(a.cache):
        ev = np.load(a.cache)
    else:
        ev = rp.column_evals(st, off, pin, d["pi"], d["exch"], optimised)
        if a.cache:
            np.save(a.cache, ev)
    evals, ncol = int(ev.sum()), int(optimised.sum())
    print("# %d loci x %d columns x %d taxa, seed %d; %d waves, grid x %d: %d columns for the optimiser (%d marked slow), %d evaluations,"
          % (a.loci, a.cols, a.taxa, a.seed, a.waves, a.grid_mult, ncol, int(slow.sum()), evals))
    print("# ideal rounds %.1f, ideal makespan %.1f rounds; histogram of evaluations %s"
          % (evals / 64.0, evals / (64.0 * a.waves), np.bincount(ev[optimised], minlength=8).tolist()))
    print("# later shares: 0 = equal column counts over waves x (grid - 1) shares; big,mid,small[,frac_big,frac_mid] = lane-fills per")
    print("# share in the three bands and the fractions of the tails that the first two take; +loci = every locus' tail begins a fresh")
    print("# fill (replay only).  shares = later shares that hold columns; makespan = the round at which the last of the waves' slots")
    print("# finishes when the shares go, in grid order, to whichever slot is free first; spread = last slot - first slot")
    print("# reserve  later shares           shares  tail cols  rounds  vs ideal  makespan  spread")
    for reserve in RESERVES:
        q = rp.fixed(reserve, rp.RESERVE_SHIFT)
        for g in GEOMETRIES + ALIGNED:
            align = g.endswith("+loci")
            tail = rp.parse_tail_shares(g.replace("+loci", ""))
            per = rp.share_rounds_work(ev, slow, optimised, off, a.waves, a.grid_mult, reserve, (2.9, 2.04), 128, True, tail, align)
            last, spread = rp.makespan(per, a.waves)
            lists = [slow[np.flatnonzero(optimised[int(off[l]):int(off[l + 1])]) + int(off[l])] for l in range(len(off) - 1)]
            tails = sum(int(rp.reserved_before(int((~m).sum()), q)) for m in lists)
            print("  %.2f     %-22s %6d  %9d  %6d  %8.4f  %8d  %6d"
                  % (reserve, g, sum(r > 0 for r in per) - a.waves, tails, sum(per), sum(per) * 64.0 / evals, last, spread))
        print()


if __name__ == "__main__":
    main()

"""Survey of short synthetic loci for the stage-1 model tests: how many of the 203 models trail the best Akaike score by more
than 21, how many end with a class rate at a bound, and the range of the fitted general-model branches.  CPU only: the host
optimiser of tapir_amd/stage1.py over the oracle's likelihood (tests/oracle_engine.py).

    python tools/stage1_locus_survey.py RATE_MEAN FIRST_SEED LAST_SEED NCOLS

Six 5-taxon loci per seed on the tree of synth.yule_tree(5, 23).  The choice of loci in tests/test_gpu_stage1_models.py rests on
runs at rate_mean 0.007 to 0.06 and 60 to 100 columns (330 loci): no model trails by 21 at that size, and a locus
with exactly one unobserved substitution type has 52 models with a rate at e^-7."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def empirical_pi(st):
    c = np.zeros(4)
    for m, n in zip(*np.unique(st, return_counts=True)):
        m = int(m) or 15
        for b in range(4):
            if (m >> b) & 1:
                c[b] += n / bin(m).count("1")
    return c / c.sum()


def main(rate_mean, first, last, ncols, nloci=6):
    import oracle_engine
    from tapir_amd import stage1, synth
    tree = synth.yule_tree(5, 23)
    pin = synth.plan_inputs(*tree)
    parent = np.asarray(pin["parent"])
    blen = np.asarray(pin["blen"]) / pin["correction"]
    for seed in range(first, last):
        d = synth.simulate(nloci, ncols, 5, seed, rate_mean=rate_mean, tree=tree)
        st = d["states"].numpy()
        pi = np.array([empirical_pi(st[:, l * ncols:(l + 1) * ncols]) for l in range(nloci)])
        t0 = time.time()
        plan = oracle_engine.Plan(5, pin["parent"], pin["blen"], pin["leaf"], d["locus_offsets"], pi, np.ones((nloci, 6)), pin["T"], [1], [[0, 1]])
        got = stage1.model_averaged_exchangeabilities(plan, st, pi, pin["parent"], blen, prune_models=False)
        _, kk = stage1.model_design(got["models"])
        score = got["lnl"] - kk[None, :]
        for l in range(nloci):
            logr = np.log(got["model_exch"][l])
            at_bound = int(((logr < -7 + 1e-6) | (logr > 9.2 - 1e-6)).any(axis=1).sum())
            br = got["grm_blen"][l][parent >= 0]
            print("rate_mean %g columns %d seed %d locus %d: trailing %d, largest gap %.2f, at a bound %d, branches %.2e .. %.2e, lnL %.2f"
                  % (rate_mean, ncols, seed, l, int((score[l] < score[l].max() - 21).sum()), score[l].max() - score[l].min(), at_bound,
                     br.min(), br.max(), got["lnl"][l, 0]), flush=True)
        print("  %.1f s" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main(float(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))

"""General-model start: the input tree's shape times a grid of scales (TPHIP_S1_START=grid) against the default, the better of
that and the per-branch parsimony counts shrunk towards it, when the input tree's branch lengths are off (each multiplied by
exp(N(0, SIGMA))) from the tree the data were simulated on.
usage: s1_start_perturbed.py LOCI COLS TAXA SIGMA"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from tapir_amd import engine, nexus, synth
L, n, nt = (int(x) for x in sys.argv[1:4])
sigma = float(sys.argv[4])
d = synth.simulate(L, n, nt, 5)
pin = synth.plan_inputs(d["root"], d["names"])
st = d["states"].numpy()
pi = nexus.base_frequencies_from_histogram(engine.state_histogram(st, d["locus_offsets"]))
rng = np.random.default_rng(3)
blen = np.asarray(pin["blen"], dtype=np.float64) * np.exp(sigma * rng.standard_normal(len(pin["blen"])))
plan = engine.Plan(nt, pin["parent"], blen, pin["leaf"], d["locus_offsets"], pi, np.ones((L, 6)), pin["T"], [1], [[0, 1]], correction=pin["correction"])
cache = plan.device_cache()
res = {}
for name in ("grid", "shrunk"):
    os.environ.pop("TPHIP_S1_START", None)
    if name == "grid":
        os.environ["TPHIP_S1_START"] = "grid"
    plan.stage1_fit(st, cache=cache)
    t0 = time.time(); out = plan.stage1_fit(st, cache=cache); dt = time.time() - t0
    res[name] = out
    print("%-5s %.3f s  general model: iterations mean %.1f max %d, gradients %d, values %d" % (name, dt, out["grm_iters"].mean(), out["grm_iters"].max(),
          out["stats"]["grm_grads"], out["stats"]["grm_evals"]), flush=True)
dl = res["shrunk"]["lnl"][:, 0] - res["grid"]["lnl"][:, 0]
rel = np.abs(res["shrunk"]["exch"] - res["grid"]["exch"]) / res["grid"]["exch"]
print("shrunk vs grid: general-model lnL better by > 1e-3 on %d loci (max %.3e), worse on %d (max %.3e); averaged rates max rel diff %.2e" % (
    (dl > 1e-3).sum(), dl.max(), (dl < -1e-3).sum(), -dl.min(), rel.max()))
cache.release(); plan.close()

"""Per-step time of the site-rate stage through the two kernels on the SAME uniform model: the GTR plan with exchangeabilities
of 1 and pi = 1/4 (eigen-system messages) and the F81 plan with pi = 1/4 (closed-form messages), on a C3-shaped synthetic
batch resident on the device.  The two alternate in one process, the device is synchronised around every timed step, and the
site-rate kernel alone is bracketed by the library's profiling events.
usage: python tools/site_model_timing.py [LOCI COLS TAXA] [reps=N]     (default 100 50000 64 = C3, reps=5)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tapir_amd import engine, synth

pos = [a for a in sys.argv[1:] if "=" not in a]
L, n, nt = (int(x) for x in pos[:3]) if len(pos) >= 3 else (100, 50000, 64)
reps = max([int(a.split("=")[1]) for a in sys.argv[1:] if a.startswith("reps=")] + [5])
d = synth.simulate(L, n, nt, 3, device="cuda")
pin = synth.plan_inputs(d["root"], d["names"])
d_states = d["states"].cuda().contiguous()
off = d["locus_offsets"]
pi = np.full((L, 4), 0.25)
dev = torch.device("cuda")
plans = {"gtr": engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, pi, np.ones((L, 6)), pin["T"], [10], [[5, 15]],
                            correction=pin["correction"]),
         "f81": engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, pi, None, pin["T"], [10], [[5, 15]],
                            correction=pin["correction"], model="f81")}
ncols = plans["gtr"].ncols
bufs = {k: dict(rate=torch.empty(ncols, dtype=torch.float64, device=dev), subst=torch.empty(ncols, dtype=torch.float64, device=dev),
                lnl=torch.empty(ncols, dtype=torch.float64, device=dev), flag=torch.empty(ncols, dtype=torch.uint8, device=dev),
                nres=torch.empty(ncols, dtype=torch.int32, device=dev),
                tables=torch.empty((L, p.width), dtype=torch.float64, device=dev),
                ws=torch.empty(p.workspace_bytes, dtype=torch.uint8, device=dev)) for k, p in plans.items()}


def step(k):
    B, p = bufs[k], plans[k]
    p.run_dev(d_states, B["rate"], B["subst"], B["lnl"], B["flag"], B["nres"], B["tables"], B["ws"],
              torch.cuda.current_stream().cuda_stream)


for k in plans:   # warm-up
    step(k)
torch.cuda.synchronize()
wall = {k: [] for k in plans}
kern = {k: [] for k in plans}
for r in range(reps):
    for k in (("gtr", "f81") if r % 2 == 0 else ("f81", "gtr")):
        p = plans[k]
        p.profile_enable(True)
        p.profile_read(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(k)
        torch.cuda.synchronize()
        wall[k].append(1e3 * (time.perf_counter() - t0))
        kern[k].append(p.profile_read(reset=True)[0])
        p.profile_enable(False)
evals = {k: p.last_eval_count() for k, p in plans.items()}
a, b = (bufs[k]["rate"].cpu().numpy() for k in ("gtr", "f81"))
fa, fb = (bufs[k]["flag"].cpu().numpy() for k in ("gtr", "f81"))
ok = (fa == 0) | (fa == 3)
rel = np.abs(a - b)[ok] / np.maximum(np.abs(a[ok]), 1e-12)
print("batch: %d loci x %d columns x %d taxa, JC model (pi = 1/4, exchangeabilities 1), %d alternating reps" % (L, n, nt, reps))
for k in plans:
    print("%s kernel: step %.3f ms (median; min %.3f), site_rate_kernel %.3f ms (median; min %.3f), evaluations %d" % (
        k, np.median(wall[k]), np.min(wall[k]), np.median(kern[k]), np.min(kern[k]), evals[k]))
print("site_rate_kernel F81 / GTR: %.3f;  step F81 / GTR: %.3f" % (np.median(kern["f81"]) / np.median(kern["gtr"]),
                                                               np.median(wall["f81"]) / np.median(wall["gtr"])))
print("flags equal: %s;  largest relative rate difference on OK/ZERO columns: %.3e" % (bool(np.array_equal(fa, fb)), rel.max()))
for p in plans.values():
    p.close()

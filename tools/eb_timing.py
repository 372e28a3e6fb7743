"""Empirical-Bayes posterior (tphip_eb_posterior_dev, the fused mixture kernel) against what the library could do for the same
numbers without it: K launches of the eval_columns diagnostic (one per rate category, u = log(mu rho_k)) and a combination
of the K [ncols] arrays (torch on the device: log-sum-exp, posterior mean and second moment).  The two alternate in one process
on one device-resident synthetic batch, timed with HIP events around each, after a warm-up; then a full fit (alpha free) of the
same batch with and without site patterns: rounds, likelihood evaluations per column, seconds per locus.
usage: python tools/eb_timing.py [LOCI COLS TAXA | R1] [reps=N] [K=4,8] [fit=0|1]     (default 100 50000 64 = C3, reps=5, K=4,8, fit=1;
R1 = the bundled real locus tests/golden/chr1_918.nex on Euteleost.tree)"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tapir_amd import eb, engine, synth

pos = [a for a in sys.argv[1:] if "=" not in a]
opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(opt.get("reps", 5))
Ks = [int(k) for k in opt.get("K", "4,8").split(",")]
if pos[:1] == ["R1"]:
    import json
    from tapir_amd import compute, newick, nexus
    g = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    names, st = nexus.read_states(os.path.join(g, "chr1_918.nex"))
    root = newick.read_tree(os.path.join(g, "Euteleost.tree"))
    depth, factor = compute.correct_tree(root)
    parent, blen, leaf = newick.to_arrays(root, names)
    kat = json.load(open(os.path.join(g, "chr1_918_phydesign_rates.json")))
    L, n, nt = 1, st.shape[1], len(names)
    d = dict(states=torch.from_numpy(np.ascontiguousarray(st)), locus_offsets=[0, n], pi=[kat["freqs_ACGT"]],
             exch=[[kat[k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]])
    pin = dict(parent=parent, blen=blen, leaf=leaf, T=int(depth), correction=factor)
else:
    L, n, nt = (int(x) for x in pos[:3]) if len(pos) >= 3 else (100, 50000, 64)
    d = synth.simulate(L, n, nt, 3, device="cuda")
    pin = synth.plan_inputs(d["root"], d["names"])
d_states = d["states"].cuda().contiguous()
states = d_states.cpu().numpy()
off = np.asarray(d["locus_offsets"])
dev = torch.device("cuda")
plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], d["exch"], pin["T"], [10], [[5, 15]],
                   correction=pin["correction"])
ncols = plan.ncols
start = eb.start_scales(states, off, pin["parent"], pin["blen"], pin["leaf"])
locus_of = torch.from_numpy(np.repeat(np.arange(L), np.diff(off))).to(dev)
kappa = torch.from_numpy(np.asarray(plan.models()[3])).to(dev)
out = {k: torch.empty(ncols, dtype=torch.float64, device=dev) for k in ("rate", "sd", "lnl")}
nres = torch.empty(ncols, dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream().cuda_stream
print("batch: %d loci x %d columns x %d taxa, %d alternating reps" % (L, n, nt, reps))
for K in Ks:
    rho, w = eb.gamma_tables(np.full(L, 1.0), K)
    d_rho = torch.from_numpy(rho).to(dev)
    d_u = [torch.log(torch.from_numpy(start * rho[:, k]).to(dev))[locus_of].contiguous() for k in range(K)]
    fgh = [[torch.empty(ncols, dtype=torch.float64, device=dev) for _ in range(3)] for _ in range(K)]
    km = (kappa * torch.from_numpy(start).to(dev))[locus_of]

    def emulate():
        for k in range(K):
            plan.eval_columns_dev(d_states, d_u[k], fgh[k][0], fgh[k][1], fgh[k][2], stream)
        f = torch.stack([fgh[k][0] for k in range(K)]) + math.log(1.0 / K)
        lnl = torch.logsumexp(f, dim=0)
        p = torch.exp(f - lnl)
        r = d_rho.t()[:, locus_of]
        mean = (p * r).sum(dim=0)
        second = (p * r * r).sum(dim=0)
        return km * mean, km * torch.sqrt(torch.clamp(second - mean * mean, min=0.0)), lnl

    def fused(patterns):
        plan.eb_posterior_dev(d_states, rho, w, start, out["rate"], out["sd"], out["lnl"], nres, use_patterns=patterns, stream=stream)

    ref = emulate()
    fused(False)
    torch.cuda.synchronize()
    print("K = %d: fused vs emulation, largest relative difference rate %.2e, lnl %.2e" % (
        K, float(((out["rate"] - ref[0]).abs() / ref[0]).max()), float(((out["lnl"] - ref[2]).abs() / ref[2].abs()).max())))
    ms = dict(emulation=[], fused=[], fused_patterns=[])
    for r in range(reps):
        order = ("emulation", "fused", "fused_patterns") if r % 2 == 0 else ("fused_patterns", "fused", "emulation")
        for which in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            emulate() if which == "emulation" else fused(which == "fused_patterns")
            b.record()
            torch.cuda.synchronize()
            ms[which].append(a.elapsed_time(b))
    for which, v in ms.items():
        print("  %-15s %.3f ms (median; min %.3f, max %.3f)" % (which, np.median(v), np.min(v), np.max(v)))
    print("  fused / emulation: %.3f" % (np.median(ms["fused"]) / np.median(ms["emulation"])))
if opt.get("fit", "1") != "0":
    for K in Ks:
        for patterns in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = eb.fit(plan, states, start, ncat=K, use_patterns=patterns)
            dt = time.perf_counter() - t0
            print("full fit K = %d patterns = %d: %.3f s = %.3f ms per locus, %d eb_fit_scale rounds, %d evaluations per column, "
                  "alpha median %.3f (%d at a bound), %d loci at the iteration limit" % (
                      K, patterns, dt, 1e3 * dt / L, f["rounds"], f["evaluations"], np.median(f["alpha"]),
                      int(np.sum((f["alpha"] < 0.2001) | (f["alpha"] > 49.99))), int(np.sum(f["iters"] < 0))))
plan.close()

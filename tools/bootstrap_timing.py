"""Site bootstrap of the PI rows (tphip_pi_bootstrap_dev: draw + matrix + summary kernels) against what a user could do for
the same bands without it: per replicate, draw the column indices on the device (torch.randint), gather the raw rates and
informative-cell counts by them and call tphip_pi_tables_dev -- B full passes of the PI stage.  The two legs alternate in one
process on one device-resident batch, each under HIP events, after a warm-up.  The rates come from one site-rate pass of the
batch itself.  The second leg is timed on min(B, emul) replicates and scaled to B (its cost is linear in B by construction).
usage: python tools/bootstrap_timing.py [C3 | C2 | R1 ...] [B=200,1000] [reps=N] [emul=N] [kernels=1]
  (default C3 C2 R1, B=200,1000, reps=3, emul=50; R1 = the bundled locus tests/golden/chr1_918.nex;
   kernels=1: one bootstrap call per shape and B and nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`)
Prints, per shape and B: ms of both legs (median, min, max), their ratio, and the arithmetic of the matrix product
(2 B n Wb flop) over the new call's whole time -- the kernel's own rate needs the kernel trace."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tapir_amd import compute, engine, newick, nexus, synth

pos = [a for a in sys.argv[1:] if "=" not in a] or ["C3", "C2", "R1"]
opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
Bs = [int(b) for b in opt.get("B", "200,1000").split(",")]
reps, emul, kernels_only = int(opt.get("reps", 3)), int(opt.get("emul", 50)), opt.get("kernels", "0") == "1"
dev = torch.device("cuda")


def batch(name):
    if name == "R1":
        g = os.path.join(ROOT, "tests", "golden")
        names, st = nexus.read_states(os.path.join(g, "chr1_918.nex"))
        root = newick.read_tree(os.path.join(g, "Euteleost.tree"))
        depth, factor = compute.correct_tree(root)
        parent, blen, leaf = newick.to_arrays(root, names)
        kat = json.load(open(os.path.join(g, "chr1_918_phydesign_rates.json")))
        d = dict(states=torch.from_numpy(np.ascontiguousarray(st)).to(dev), pi=[kat["freqs_ACGT"]],
                 exch=[[kat[k] for k in ("AC", "AG", "AT", "CG", "CT", "GT")]])
        pin = dict(parent=parent, blen=blen, leaf=leaf, T=int(depth), correction=factor)
        return d, pin, 1, st.shape[1], len(names), [10, 30, 50, 90], [[5, 15], [25, 35], [45, 55], [85, 95]]
    L, n, nt, times, intervals = synth.WORKLOADS[name]
    d = synth.simulate(L, n, nt, synth.WORKLOAD_SEED[name], device=dev, tree=synth.yule_tree(nt, synth.WORKLOAD_SEED[name]))
    return d, synth.plan_inputs(d["root"], d["names"]), L, n, nt, times, intervals


for name in pos:
    d, pin, L, n, nt, times, intervals = batch(name)
    off = np.arange(L + 1, dtype=np.int64) * n
    plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], d["exch"], pin["T"], times, intervals,
                       correction=pin["correction"], threshold=3, round_decimals=4)
    ncols, Wb = plan.ncols, plan.bootstrap_width
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
    rate, subst, lnl = f64(ncols), f64(ncols), f64(ncols)
    flag, nres = torch.empty(ncols, dtype=torch.uint8, device=dev), torch.empty(ncols, dtype=torch.int32, device=dev)
    tables, ws = f64(L, plan.width), torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    plan.run_dev(d["states"].contiguous(), rate, subst, lnl, flag, nres, tables, ws, stream)
    torch.cuda.synchronize()
    base = torch.from_numpy(off[:-1]).to(dev)[:, None]
    g_rate, g_nres, g_tab = f64(ncols), torch.empty_like(nres), f64(L, plan.width)
    print("%s: %d loci x %d columns, T = %d, %d intervals, Wb = %d" % (name, L, n, pin["T"], len(intervals), Wb))
    for B in Bs:
        mn, pf = plan.bootstrap_workspace_bytes(B)
        bws = torch.empty(pf, dtype=torch.uint8, device=dev)
        summary = f64(L, 4, Wb)

        def new_call():
            plan.pi_bootstrap_dev(rate, nres, summary, None, bws, B, seed=1, stream=stream)

        def emulation(k):
            for _ in range(k):
                idx = (torch.randint(0, n, (L, n), device=dev) + base).reshape(-1)
                torch.index_select(rate, 0, idx, out=g_rate)
                torch.index_select(nres, 0, idx, out=g_nres)
                plan.pi_tables_dev(g_rate, g_nres, g_tab, ws, stream)

        if kernels_only:
            new_call()
            torch.cuda.synchronize()
            continue
        k = min(B, emul)
        new_call()
        emulation(2)
        torch.cuda.synchronize()
        ms = dict(bootstrap=[], emulation=[])
        for r in range(reps):
            for which in (("bootstrap", "emulation") if r % 2 == 0 else ("emulation", "bootstrap")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                new_call() if which == "bootstrap" else emulation(k)
                b.record()
                torch.cuda.synchronize()
                ms[which].append(a.elapsed_time(b) * (1.0 if which == "bootstrap" else B / k))
        point = tables[:, :pin["T"]]
        rel = float(((summary[:, 0, :pin["T"]] - point).abs() / point.clamp(min=1e-300))[:, 1:].max())
        flop = 2.0 * B * ncols * Wb
        for which, v in ms.items():
            print("  B = %4d %-10s %10.3f ms (median; min %.3f, max %.3f)%s" % (
                B, which, np.median(v), np.min(v), np.max(v), "" if which == "bootstrap" else "   [%d replicates timed, scaled]" % k))
        print("  B = %4d emulation / bootstrap = %.2f; workspace %.1f MB (min %.1f MB); matrix arithmetic %.3g flop = %.2f TF over the "
              "whole call; largest |mean - point| / point = %.3g" % (
                  B, np.median(ms["emulation"]) / np.median(ms["bootstrap"]), pf / 1e6, mn / 1e6, flop,
                  flop / (np.median(ms["bootstrap"]) * 1e-3) / 1e12, rel))
        del bws
    plan.close()

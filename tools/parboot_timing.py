"""Parametric bootstrap on a device-resident batch, after a warm-up:
  * simulate_columns_kernel per replicate under HIP events (tphip_simulate_columns_dev with the observed alignment as mask),
    median of `runs` runs of `per_run` launches each, and its columns per second;
  * the only earlier route to a simulated alignment, synth.simulate(device="cuda") of the same shape (torch, three full-tensor
    passes per tree node), host clock around a device synchronise, median of `runs` runs, and the ratio of the two rates with
    the spread of both;
  * the site-rate stage per replicate inside the whole call, from the plan's profiling hooks;
  * the whole tphip_pi_parametric_bootstrap_dev call of B replicates under HIP events.
The rates the simulation runs at come from one site-rate pass of the batch itself.
usage: python tools/parboot_timing.py [C3 | C2 ...] [B=100] [runs=5] [per_run=10] [synth=1]

Work of the simulate kernel per column, counted from csrc/simulate_kernels.hpp for a tree of N nodes and n taxa under GTR:
(N - 1) x 3 expm1 (F81: 1), half a Philox call per node, one LDS read per non-root node and one LDS write per internal node;
bytes: 8 (rate) + n (mask) + n (output)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    import torch
    from tapir_amd import engine, synth
    pos = [a for a in sys.argv[1:] if "=" not in a] or ["C3", "C2"]
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    B, runs, per_run = int(opt.get("B", 100)), int(opt.get("runs", 5)), int(opt.get("per_run", 10))
    do_synth = opt.get("synth", "1") == "1"
    dev = torch.device("cuda")
    for name in pos:
        L, n, nt, times, intervals = synth.WORKLOADS[name]
        seed = synth.WORKLOAD_SEED[name]
        tree = synth.yule_tree(nt, seed)
        d = synth.simulate(L, n, nt, seed, device=dev, tree=tree)
        pin = synth.plan_inputs(d["root"], d["names"])
        off = np.arange(L + 1, dtype=np.int64) * n
        plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], d["exch"], pin["T"], times, intervals,
                           correction=pin["correction"], threshold=3, round_decimals=4)
        ncols, nnodes = plan.ncols, len(pin["parent"])
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
        observed = d["states"].contiguous()
        rate, subst, lnl = f64(ncols), f64(ncols), f64(ncols)
        flag, nres = torch.empty(ncols, dtype=torch.uint8, device=dev), torch.empty(ncols, dtype=torch.int32, device=dev)
        tables, ws = f64(L, plan.width), torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        plan.run_dev(observed, rate, subst, lnl, flag, nres, tables, ws, stream)
        torch.cuda.synchronize()
        print("%s: %d loci x %d columns, %d taxa (%d nodes), B = %d" % (name, L, n, nt, nnodes, B))

        # 1. the simulate kernel alone
        sim_out = torch.empty_like(observed)
        plan.simulate_columns_dev(rate, observed, sim_out, replicate=0, seed=1, stream=stream)      # warm-up
        torch.cuda.synchronize()
        sim_ms = []
        for r in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(per_run):
                plan.simulate_columns_dev(rate, observed, sim_out, replicate=r * per_run + k, seed=1, stream=stream)
            b.record()
            torch.cuda.synchronize()
            sim_ms.append(a.elapsed_time(b) / per_run)
        med = float(np.median(sim_ms))
        sim_cps = [ncols / (m * 1e-3) for m in sim_ms]
        print("  simulate_columns_kernel  %9.3f ms per replicate (median of %d runs of %d; min %.3f, max %.3f) = %.3e columns/s"
              % (med, runs, per_run, min(sim_ms), max(sim_ms), ncols / (med * 1e-3)))
        print("    per column: %d expm1, %.1f Philox calls, %d bytes read, %d written = %.2e expm1/s, %.1f GB/s"
              % (3 * (nnodes - 1), nnodes / 2.0, 8 + nt, nt, 3 * (nnodes - 1) * ncols / (med * 1e-3),
                 (8 + 2 * nt) * ncols / (med * 1e-3) / 1e9))

        # 2. the earlier route: the torch generator of the benchmark inputs
        if do_synth:
            synth.simulate(L, n, nt, seed, device=dev, tree=tree)      # warm-up
            torch.cuda.synchronize()
            sec = []
            for r in range(runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                synth.simulate(L, n, nt, seed + 1 + r, device=dev, tree=tree)
                torch.cuda.synchronize()
                sec.append(time.perf_counter() - t0)
            smed = float(np.median(sec))
            syn_cps = [ncols / s for s in sec]
            print("  synth.simulate(device=cuda) %9.3f ms per alignment (median of %d; min %.3f, max %.3f) = %.3e columns/s"
                  % (smed * 1e3, runs, min(sec) * 1e3, max(sec) * 1e3, ncols / smed))
            print("    ratio of the medians %.1f x; slowest kernel run over fastest synth run %.1f x (columns/s: kernel %.3e..%.3e, "
                  "synth %.3e..%.3e)" % (smed * 1e3 / med, min(sim_cps) / max(syn_cps), min(sim_cps), max(sim_cps), min(syn_cps),
                                         max(syn_cps)))

        # 3. the whole call, with the site-rate stage bracketed by the plan's profiling hooks
        Wb = plan.bootstrap_width
        summary, mean, sd = f64(L, 4, Wb), f64(ncols), f64(ncols)
        pws = torch.empty(plan.parboot_workspace_bytes(B), dtype=torch.uint8, device=dev)
        plan.pi_parametric_bootstrap_dev(rate, observed, summary, None, mean, sd, pws, 2, seed=1, stream=stream)      # warm-up
        torch.cuda.synchronize()
        plan.profile_enable(True)
        plan.profile_read(reset=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan.pi_parametric_bootstrap_dev(rate, observed, summary, None, mean, sd, pws, B, seed=1, stream=stream)
        b.record()
        torch.cuda.synchronize()
        whole = a.elapsed_time(b)
        site_ms, pi_ms, launches = plan.profile_read(reset=True)
        plan.profile_enable(False)
        print("  tphip_pi_parametric_bootstrap_dev  %9.1f ms for B = %d = %.3f ms per replicate (workspace %.0f MiB)"
              % (whole, B, whole / B, pws.numel() / 2 ** 20))
        print("    site-rate kernel %.3f ms per replicate (%d launches), PI kernels %.3f ms per replicate; simulate kernel %.3f ms "
              "(from 1.) = %.0f %% of the site-rate kernel it feeds" % (site_ms / max(launches, 1), launches, pi_ms / max(launches, 1),
                                                                        med, 100 * med / max(site_ms / max(launches, 1), 1e-9)))
        m, s = mean.cpu().numpy(), sd.cpu().numpy()
        fin = np.isfinite(m)
        print("    rate moments: %d of %d columns not culled; mean of the means %.4g, mean sd %.4g" % (fin.sum(), ncols, m[fin].mean(), s[fin].mean()))
        plan.close()
        del d, observed, sim_out, rate, subst, lnl, flag, nres, tables, ws, pws, summary, mean, sd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

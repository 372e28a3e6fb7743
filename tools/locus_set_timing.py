"""Locus-set accumulation curves (tphip_locus_set_exact_dev: locus_set_moment_kernel + locus_set_head_kernel +
locus_set_spectrum_kernel + locus_set_finalise_kernel, and tphip_locus_set_rows_dev) on device-resident
per-site planes under HIP events, after a warm-up, beside tphip_quartet_exact_dev at the same cap on the same planes.  The
rates come from one site-rate pass of the batch itself; the order is the default one (descending per-locus p_correct).
usage: python tools/locus_set_timing.py [C2 ...] [nq=100] [reps=3] [caps=128,512]
  quartets: T = 1..nq (one per integer), all with t_o = 5
Prints, per shape and cap: the head lengths (prefixes computed per quartet), ms of the call (median, min, max), the (site,
frequency) products of the heads' live sites on the torus of the cap and their rate per second, and the same for
tphip_quartet_exact_dev (whose pairs choose their own window up to the cap)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _timed(fn, reps):
    import torch
    fn()                                                       # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), min(ms), max(ms)


def main():
    import torch
    from tapir_amd import engine, pipeline, synth
    pos = [a for a in sys.argv[1:] if "=" not in a] or ["C2"]
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    nq, reps = int(opt.get("nq", 100)), int(opt.get("reps", 3))
    caps = [int(c) for c in opt.get("caps", "128,512").split(",")]
    quartets = np.array([[float(t), 5.0] for t in range(1, nq + 1)])
    dev = torch.device("cuda")
    for name in pos:
        L, n, nt, times, intervals = synth.WORKLOADS[name]
        d = synth.simulate(L, n, nt, synth.WORKLOAD_SEED[name], device=dev, tree=synth.yule_tree(nt, synth.WORKLOAD_SEED[name]))
        pin = synth.plan_inputs(d["root"], d["names"])
        off = np.arange(L + 1, dtype=np.int64) * n
        plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], d["exch"], pin["T"], times, intervals,
                           correction=pin["correction"], threshold=3, round_decimals=4)
        ncols = plan.ncols
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
        rate, subst, lnl = f64(ncols), f64(ncols), f64(ncols)
        flag, nres = torch.empty(ncols, dtype=torch.uint8, device=dev), torch.empty(ncols, dtype=torch.int32, device=dev)
        tables, ws = f64(L, plan.width), torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        plan.run_dev(d["states"].contiguous(), rate, subst, lnl, flag, nres, tables, ws, stream)
        torch.cuda.synchronize()
        sites = f64(2, nq, ncols)
        rows8 = f64(L, nq, 8)
        qws = torch.empty(plan.quartet_workspace_bytes(quartets), dtype=torch.uint8, device=dev)
        plan.quartet_sites_dev(rate, nres, quartets, sites, stream)
        plan.quartet_tables_dev(rate, nres, quartets, rows8, qws, stream)
        torch.cuda.synchronize()
        live = ((sites[0] != 0) | (sites[1] != 0)).reshape(nq, L, n).sum(dim=2).T.cpu().numpy().astype(np.float64)   # [L, nq]
        order = pipeline.locus_set_order(rows8.cpu().numpy(), ["l%d" % l for l in range(L)])
        K = order.shape[1]
        print("%s: %d loci x %d columns, %d quartets (T = 1..%d, t_o = 5), the default order of all %d loci: %.3e live (site, "
              "quartet) pairs" % (name, L, n, nq, nq, K, live.sum()))
        set_rows = f64(nq, K, 8)
        t = _timed(lambda: engine.locus_set_rows_dev(rows8, L, order, set_rows, stream=stream), reps)
        print("  tphip_locus_set_rows_dev        %10.3f ms (median of %d; min %.3f, max %.3f)  [the normal rows, %d per quartet]"
              % (t[0], reps, t[1], t[2], K))
        for cap in caps:
            freq = cap * (cap // 2 + 1)
            rows = f64(nq, K, 6)
            lws = torch.empty(plan.locus_set_exact_workspace_bytes(nq, K, cap), dtype=torch.uint8, device=dev)
            t = _timed(lambda: plan.locus_set_exact_dev(sites[0], sites[1], sites[1], order, rows, lws, cap, 0.0, 0, stream), reps)
            got = rows.cpu().numpy()
            heads = (got[..., 4] != 0).sum(axis=1)
            products = float(sum(live[order[q, :heads[q]], q].sum() for q in range(nq))) * freq
            print("  tphip_locus_set_exact_dev cap %3d %9.3f ms (median of %d; min %.3f, max %.3f); workspace %.1f MB"
                  % (cap, t[0], reps, t[1], t[2], lws.numel() / 1e6))
            print("    head lengths: min %d, median %d, max %d, sum %d of %d prefixes; %.3e (site, frequency) products = %.3e /s; "
                  "%.1f boundaries with a weight refill per workgroup and tile"
                  % (heads.min(), int(np.median(heads)), heads.max(), heads.sum(), nq * K, products, products / (t[0] * 1e-3),
                     heads.mean()))
            done = got[..., 4] != 0
            if done.any():
                print("    rows sum to 1 within %.1e; p_correct of the longest computed set: min %.4f, max %.4f"
                      % (np.abs(got[..., :4].sum(axis=-1)[done] - 1).max(),
                         min(got[q, heads[q] - 1, 0] for q in range(nq) if heads[q]), max(got[q, heads[q] - 1, 0] for q in range(nq) if heads[q])))
            del rows, lws
            erows = f64(L, nq, 6)
            ews = torch.empty(plan.quartet_exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=dev)
            t = _timed(lambda: plan.quartet_exact_dev(sites[0], sites[1], sites[1], nq, erows, ews, cap, 0.0, stream), reps)
            win = erows.cpu().numpy()[..., 4]
            eprod = float((live * win * (win / 2 + 1))[win > 0].sum())
            print("  tphip_quartet_exact_dev   cap %3d %9.3f ms (median of %d; min %.3f, max %.3f): %.3e products = %.3e /s  [every "
                  "locus alone, its own window]" % (cap, t[0], reps, t[1], t[2], eprod, eprod / (t[0] * 1e-3)))
            del erows, ews
        plan.close()
        del d, rate, subst, lnl, flag, nres, tables, ws, sites, rows8, qws, set_rows
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

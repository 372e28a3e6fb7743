"""The exact quartet resolution probabilities (tphip_quartet_exact_dev: exact_moment_kernel + exact_spectrum_kernel +
exact_finalise_kernel) on device-resident per-site planes under HIP events, after a warm-up, beside the
call that writes the planes (tphip_quartet_sites_dev) and the normal approximation's own call (tphip_quartet_tables_dev).
The rates come from one site-rate pass of the batch itself.  There is no earlier path to compare with.
usage: python tools/exact_quartet_timing.py [C2 | C3 ...] [nq=100] [reps=3] [caps=128,512]
  quartets: T = 1..nq (one per integer), all with t_o = 5
Prints, per shape and cap: ms of the call (median, min, max), the share of (locus, quartet) pairs computed and their windows,
(site, frequency) products per second over the live sites of the computed pairs, and the flop rate by the source-counted
model below with its fraction of the 78.6 TF FP64 vector peak.

Flop model, counted from csrc/exact_quartet_kernels.hpp (an fma is 2): per live site and frequency the factor is 3 fma
(real part) + 1 mul and 2 fma (imaginary part) = 11, the complex product 2 mul + 2 fma = 6: 17 flop in 10 instructions.  A pair
of window M has M (M / 2 + 1) frequencies; twiddles, weights and the moment pass are left out."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

FLOP_PER_SITE_FREQ = 17.0
PEAK_TF = 78.6


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
    from tapir_amd import engine, synth
    pos = [a for a in sys.argv[1:] if "=" not in a] or ["C2", "C3"]
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
        t_sites = _timed(lambda: plan.quartet_sites_dev(rate, nres, quartets, sites, stream), reps)
        t_norm = _timed(lambda: plan.quartet_tables_dev(rate, nres, quartets, rows8, qws, stream), reps)
        live = ((sites[0] != 0) | (sites[1] != 0)).reshape(nq, L, n).sum(dim=2).T.cpu().numpy().astype(np.float64)   # [L, nq]
        print("%s: %d loci x %d columns, %d quartets (T = 1..%d, t_o = 5): %d pairs, %.3e live (site, quartet) pairs"
              % (name, L, n, nq, nq, L * nq, live.sum()))
        print("  tphip_quartet_sites_dev   %10.3f ms (median of %d; min %.3f, max %.3f)  [writes the planes, %.2f GB]"
              % (t_sites[0], reps, t_sites[1], t_sites[2], 2 * nq * ncols * 8 / 1e9))
        print("  tphip_quartet_tables_dev  %10.3f ms (median of %d; min %.3f, max %.3f)  [the normal approximation]"
              % (t_norm[0], reps, t_norm[1], t_norm[2]))
        normal = rows8.cpu().numpy()
        for cap in caps:
            rows = f64(L, nq, 6)
            ews = torch.empty(plan.quartet_exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=dev)
            t = _timed(lambda: plan.quartet_exact_dev(sites[0], sites[1], sites[1], nq, rows, ews, cap, 0.0, stream), reps)
            got = rows.cpu().numpy()
            win = got[..., 4]
            done = win > 0
            products = float((live * win * (win / 2 + 1))[done].sum())
            tf = products * FLOP_PER_SITE_FREQ / (t[0] * 1e-3) / 1e12
            hist = ", ".join("%d: %d" % (m, int((win == m).sum())) for m in (16, 32, 64, 128, 256, 512) if (win == m).any())
            print("  tphip_quartet_exact_dev cap %3d  %10.3f ms (median of %d; min %.3f, max %.3f); workspace %.1f MB"
                  % (cap, t[0], reps, t[1], t[2], ews.numel() / 1e6))
            print("    computed %d of %d pairs = %.1f %% (windows %s); %.3e (site, frequency) products = %.3e /s; at %.0f flop "
                  "each %.2f TF = %.1f %% of the %.1f TF FP64 peak"
                  % (done.sum(), done.size, 100.0 * done.mean(), hist or "none", products, products / (t[0] * 1e-3),
                     FLOP_PER_SITE_FREQ, tf, 100 * tf / PEAK_TF, PEAK_TF))
            if done.any():
                gap = np.abs(np.stack([got[..., 0] - normal[..., 5], got[..., 1] + got[..., 2] - normal[..., 6],
                                       got[..., 3] - normal[..., 7]]))[:, done]
                print("    exact minus normal approximation over the computed pairs: largest %.4f, mean %.4f; rows sum to 1 within %.1e"
                      % (gap.max(), gap.mean(), np.abs(got[..., :4].sum(axis=-1)[done] - 1).max()))
            del rows, ews
        plan.close()
        del d, rate, subst, lnl, flag, nres, tables, ws, sites, rows8, qws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

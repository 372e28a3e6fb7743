"""The empirical-Bayes rate posterior carried into the PI rows under HIP events, after a warm-up: the table
call (tphip_eb_posterior_table_dev) beside the call it extends (tphip_eb_posterior_dev: what the table adds is the store of K
doubles per column and the normalisation), and the draw call (tphip_posterior_pi_dev: category rows, moments, B x ncols
categorical draws, rows, summary) beside the site bootstrap of the same batch at the same B (tphip_pi_bootstrap_dev).
Every locus is evaluated at the engine's own start scale with alpha = 1.
usage: python tools/posterior_pi_timing.py [C2 | C3 ...] [K=8] [B=1000] [reps=3]
Prints, per shape: ms of each call (median, min, max) and the draw call's draws per second."""
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
    from tapir_amd import eb, engine, synth
    pos = [a for a in sys.argv[1:] if "=" not in a] or ["C2", "C3"]
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    K, B, reps = int(opt.get("K", 8)), int(opt.get("B", 1000)), int(opt.get("reps", 3))
    dev = torch.device("cuda")
    for name in pos:
        L, n, nt, times, intervals = synth.WORKLOADS[name]
        d = synth.simulate(L, n, nt, synth.WORKLOAD_SEED[name], device=dev, tree=synth.yule_tree(nt, synth.WORKLOAD_SEED[name]))
        pin = synth.plan_inputs(d["root"], d["names"])
        off = np.arange(L + 1, dtype=np.int64) * n
        plan = engine.Plan(nt, pin["parent"], pin["blen"], pin["leaf"], off, d["pi"], d["exch"], pin["T"], times, intervals,
                           correction=pin["correction"], threshold=3, round_decimals=4)
        ncols, Wb = plan.ncols, plan.bootstrap_width
        states = d["states"].contiguous()
        stream = torch.cuda.current_stream().cuda_stream
        f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
        rate, sd, lnl, post = f64(ncols), f64(ncols), f64(ncols), f64(K, ncols)
        nres = torch.empty(ncols, dtype=torch.int32, device=dev)
        scale = plan.eb_start_scale_dev(states, stream)
        rho, w = eb.gamma_tables(np.ones(L), K)
        t_plain = _timed(lambda: plan.eb_posterior_dev(states, rho, w, scale, rate, sd, lnl, nres, stream=stream), reps)
        t_table = _timed(lambda: plan.eb_posterior_table_dev(states, rho, w, scale, post, rate, sd, lnl, nres, stream=stream), reps)
        d_scale, d_rho = torch.from_numpy(scale).to(dev), torch.from_numpy(np.ascontiguousarray(rho)).to(dev)
        analytic, expected, summary = f64(L, 2, Wb), f64(L, K), f64(L, 4, Wb)
        ws = torch.empty(plan.posterior_pi_workspace_bytes(K, B)[1], dtype=torch.uint8, device=dev)
        t_draw = _timed(lambda: plan.posterior_pi_dev(post, nres, d_scale, d_rho, K, analytic, expected, summary, None, None, ws, B,
                                                      stream=stream), reps)
        bws = torch.empty(plan.bootstrap_workspace_bytes(B)[1], dtype=torch.uint8, device=dev)
        bsum = f64(L, 4, Wb)
        t_boot = _timed(lambda: plan.pi_bootstrap_dev(rate, nres, bsum, None, bws, B, stream=stream), reps)
        live = int((nres >= 3).sum().item())
        print("%s: %d loci x %d columns, %d taxa, K = %d, B = %d, Wb = %d (%d of %d columns live)" % (name, L, n, nt, K, B, Wb, live, ncols))
        line = "  %-30s %10.3f ms (median of %d; min %.3f, max %.3f)%s"
        print(line % ("tphip_eb_posterior_dev", t_plain[0], reps, t_plain[1], t_plain[2], ""))
        print(line % ("tphip_eb_posterior_table_dev", t_table[0], reps, t_table[1], t_table[2],
                      "  [%.3f x; the table: %.2f GB]" % (t_table[0] / t_plain[0], K * ncols * 8 / 1e9)))
        print(line % ("tphip_posterior_pi_dev", t_draw[0], reps, t_draw[1], t_draw[2],
                      "  [%.3e draws = %.3e /s; workspace %.1f MB]" % (float(B) * ncols, float(B) * ncols / (t_draw[0] * 1e-3),
                                                                        ws.numel() / 1e6)))
        print(line % ("tphip_pi_bootstrap_dev", t_boot[0], reps, t_boot[1], t_boot[2], "  [workspace %.1f MB]" % (bws.numel() / 1e6)))
        sm = summary.cpu().numpy()
        an = analytic.cpu().numpy()
        z = np.abs(sm[:, 0, 1:] - an[:, 0, 1:]) / np.maximum(an[:, 1, 1:] / np.sqrt(B), 1e-300)
        print("  draws against the analytic moments: largest |mean of draws - mean| in standard errors %.2f" % z[an[:, 1, 1:] > 0].max())
        plan.close()
        del d, states, rate, sd, lnl, post, nres, ws, bws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

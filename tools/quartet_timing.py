"""Quartet signal and noise (tphip_quartet_tables_dev: quartet_partial_kernel + quartet_reduce_kernel) on a device-resident
batch under HIP events, after a warm-up, and -- in the same run -- the fp64 numpy restatement of the same formulas
(tests/quartet_reference.py) on 16 CPU processes for a subsample of the same (site, quartet) pairs, extrapolated to all of
them.  There is no earlier path to compare with: the CPU line is what a user could do without the kernels.
The rates come from one site-rate pass of the batch itself.
usage: python tools/quartet_timing.py [C3 | C2 ...] [nq=100] [reps=3] [cpu_sites=4000] [cpu_quartets=10] [cpu=1]
  quartets: T = 1..nq (one per integer), all with t_o = 5
Prints, per shape: ms of the call (median, min, max), (site, quartet) pairs per second, the flop rate by the source-counted
model below and its fraction of the 78.6 TF FP64 vector peak, then the CPU line.

Flop model, counted from csrc/quartet_kernels.hpp (an fma is 2; the library's expm1 is counted as calls, not as flop):
  quartet_transition (GTR)   2 (s) + 3 (lam s) + 12 (U e) + 16 x 5 (entries) + 4 (diagonal) = 101 flop and 3 expm1
  quartet_signal_noise       16 (squares) + 32 (R) + 16 x 10 (signal) + 22 + 40 + 80 + 30 (noise) = 380 flop
  five running sums          8 flop
  this list (every T its own, one t_o): M per pair, N once per tile of 4 quartets: 1.25 x 101 + 380 + 8 = 514 flop and
  3.75 expm1 per live (site, quartet) pair; a culled or zero-rate column costs nothing."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

FLOP_PER_PAIR = 1.25 * 101 + 380 + 8
PEAK_TF = 78.6


def _cpu_share(job):
    """one process' share of the subsample: the restatement's per-site values and their five sums"""
    import quartet_reference as qr
    pi, exch, rates, quartets = job
    out = []
    for tip, internode in quartets:
        y, x = qr.site_values("gtr", pi, exch, rates, tip, internode)
        out.append(qr.locus_sums(y, x))
    return out


def main():
    import torch
    from tapir_amd import engine, synth
    pos = [a for a in sys.argv[1:] if "=" not in a] or ["C3", "C2"]
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    nq, reps = int(opt.get("nq", 100)), int(opt.get("reps", 3))
    cpu_sites, cpu_quartets, do_cpu = int(opt.get("cpu_sites", 4000)), int(opt.get("cpu_quartets", 10)), opt.get("cpu", "1") == "1"
    quartets = np.array([[float(t), 5.0] for t in range(1, nq + 1)])
    dev = torch.device("cuda")
    pool = None
    if do_cpu:   # spawned before the GPU work of this process begins; the workers never touch the GPU
        import multiprocessing as mp
        pool = mp.get_context("spawn").Pool(16)
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
        fin = plan_final_rates(rate.cpu().numpy(), nres.cpu().numpy(), pin["correction"])
        live = int(np.count_nonzero(np.isfinite(fin) & (fin != 0.0)))
        rows = f64(L, nq, 8)
        qws = torch.empty(plan.quartet_workspace_bytes(quartets), dtype=torch.uint8, device=dev)
        plan.quartet_tables_dev(rate, nres, quartets, rows, qws, stream)      # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            plan.quartet_tables_dev(rate, nres, quartets, rows, qws, stream)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = float(np.median(ms))
        pairs, live_pairs = float(ncols) * nq, float(live) * nq
        tf = live_pairs * FLOP_PER_PAIR / (med * 1e-3) / 1e12
        got = rows.cpu().numpy()
        print("%s: %d loci x %d columns (%d live: non-zero, not culled), %d quartets (T = 1..%d, t_o = 5)" % (name, L, n, live, nq, nq))
        print("  tphip_quartet_tables_dev  %10.3f ms (median of %d; min %.3f, max %.3f)" % (med, reps, min(ms), max(ms)))
        print("  %.3e (site, quartet) pairs/s over all columns, %.3e over the live ones; %.0f flop per live pair (source-counted, "
              "expm1 not included) = %.2f TF = %.1f %% of the %.1f TF FP64 peak; %.2e expm1/s"
              % (pairs / (med * 1e-3), live_pairs / (med * 1e-3), FLOP_PER_PAIR, tf, 100 * tf / PEAK_TF, PEAK_TF,
                 3.75 * live_pairs / (med * 1e-3)))
        print("  locus 0: p_correct at T = 1, %d, %d: %.4f %.4f %.4f; p_incorrect %.4f %.4f %.4f"
              % (nq // 2, nq, got[0, 0, 5], got[0, nq // 2 - 1, 5], got[0, nq - 1, 5], got[0, 0, 6], got[0, nq // 2 - 1, 6], got[0, nq - 1, 6]))
        if pool is not None:
            # the subsample: the first cpu_sites columns of locus 0 under every (nq / cpu_quartets)-th quartet, dealt over 16 processes
            m = min(cpu_sites, n)
            sub_q = quartets[::max(1, nq // cpu_quartets)][:cpu_quartets]
            pi0, ex0 = np.asarray(d["pi"][0], dtype=np.float64), np.asarray(d["exch"][0], dtype=np.float64)
            shares = [(pi0, ex0, fin[k:m:16], sub_q) for k in range(16)]
            pool.map(_cpu_share, shares[:16])                                     # warm-up: imports, first calls
            t0 = time.perf_counter()
            res = pool.map(_cpu_share, shares)
            sec = time.perf_counter() - t0
            sub_pairs = float(m) * len(sub_q)
            total = np.sum([np.array(r) for r in res], axis=0)
            qi = [int(np.flatnonzero((quartets == q).all(axis=1))[0]) for q in sub_q]
            print("  numpy restatement, 16 processes: %.3f s for %d x %d = %.3e pairs = %.3e pairs/s; EXTRAPOLATED to all %.3e pairs: "
                  "%.1f s = %.0f x the GPU call" % (sec, m, len(sub_q), sub_pairs, sub_pairs / sec, pairs, pairs / (sub_pairs / sec),
                                                    pairs / (sub_pairs / sec) / (med * 1e-3)))
            if m == n:
                rel = np.abs(got[0, qi, :2] - total[:, :2]) / np.maximum(total[:, :2], 1e-300)
                print("  locus 0, those quartets: GPU sums against the restatement's, largest relative difference %.2e" % rel.max())
        plan.close()
        del d, rate, subst, lnl, flag, nres, tables, ws, rows, qws
        torch.cuda.empty_cache()
    if pool is not None:
        pool.close()
        pool.join()


def plan_final_rates(rate, nres, correction):
    """what finalize_rate gives for a round_decimals = 4, threshold = 3 plan (host copy, for the CPU line and the live count)"""
    from tapir_amd import compute
    r = compute.round_like_hyphy(rate, 4) / correction
    return np.where(nres >= 3, r, np.nan)


if __name__ == "__main__":
    main()

"""Quartets with unequal tips (tphip_unequal_quartet_tables_dev: uquartet_partial_kernel + uquartet_reduce_kernel) on a
device-resident batch under HIP events, after a warm-up, and -- in the same process, on the same rates, at the same number
of quartets -- the equal-tip call tphip_quartet_tables_dev, which is the yardstick (DESIGN.md sections 3.6 and 3.8).
The rates come from one site-rate pass of the batch itself.
usage: python tools/unequal_quartet_timing.py [C3 | C2 ...] [taxa=64] [reps=3]
  quartets: the taxa - 3 internodes of synth.yule_tree(taxa, 20261006) by compute.tree_quartets (nearest tips); the equal-tip
  call gets (Ta, t_o) of the same internodes: every T and every t_o its own, so neither call reuses a matrix
Prints, per shape and call: ms (median, min, max), (site, quartet) pairs per second over all and over the live columns, the
flop rate by the source-counted models below, and the ratio of the two calls next to the ratio of their counted flop.

Flop models (an fma is 2; the library's expm1 is counted as calls, not as flop), per live (site, quartet) pair:
  unequal tips, counted from csrc/unequal_quartet_kernels.hpp (GTR)
    five scales 10 + five times three eigenvalue products 15 + the rows of C and D 8 x 24 = 192
    per root state u: rows of A, B, N 72 + n C 16 + R_u 16 x 7 = 112 + signal 21 + noise 12 x 6 + 4 = 76: 297, four times 1188
    nine running sums 15
    = 1420 flop and 15 expm1; a quartet with Ta = Tb (every one of an ultrametric tree, so every one of this list) takes B's
    exponentials from A: 1415 flop and 12 expm1
  equal tips, tools/quartet_timing.py's count with M and N both made per pair: 2 x 101 + 380 + 8 = 590 flop and 6 expm1
A culled or zero-rate column costs nothing in either."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

FLOP_UNEQUAL, EXPM1_UNEQUAL = 10 + 15 + 192 + 4 * 297 + 15 - 5, 12   # (Ta = Tb throughout the list)
FLOP_EQUAL, EXPM1_EQUAL = 2 * 101 + 380 + 8, 6
PEAK_TF = 78.6


def _timed(call, reps):
    import torch
    call()                                                                   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    import torch
    from tapir_amd import compute, engine, synth
    pos = [a for a in sys.argv[1:] if "=" not in a] or ["C3", "C2"]
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    taxa, reps = int(opt.get("taxa", 64)), int(opt.get("reps", 3))
    of_tree = compute.tree_quartets(synth.yule_tree(taxa, 20261006)[0])
    unequal = np.array([q[2:] for q in of_tree], dtype=np.float64)
    equal = np.ascontiguousarray(unequal[:, [0, 4]])
    assert np.all(unequal[:, 0] == unequal[:, 1])                                # what the flop model above counts on
    nq = len(unequal)
    dev = torch.device("cuda")
    print("device %s; %d quartets of a %d-taxon Yule tree: tips %.3g .. %.3g, internodes %.3g .. %.3g"
          % (torch.cuda.get_device_name(0), nq, taxa, unequal[:, :4].min(), unequal[:, :4].max(), unequal[:, 4].min(), unequal[:, 4].max()))
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
        fin = np.where(nres.cpu().numpy() >= 3, compute.round_like_hyphy(rate.cpu().numpy(), 4) / pin["correction"], np.nan)
        live = int(np.count_nonzero(np.isfinite(fin) & (fin != 0.0)))
        urows, erows = f64(L, nq, 13), f64(L, nq, 8)
        uws = torch.empty(plan.unequal_quartet_workspace_bytes(unequal), dtype=torch.uint8, device=dev)
        ews = torch.empty(plan.quartet_workspace_bytes(equal), dtype=torch.uint8, device=dev)
        ms_u = _timed(lambda: plan.unequal_quartet_tables_dev(rate, nres, unequal, urows, uws, stream), reps)
        ms_e = _timed(lambda: plan.quartet_tables_dev(rate, nres, equal, erows, ews, stream), reps)
        pairs, live_pairs = float(ncols) * nq, float(live) * nq
        print("%s: %d loci x %d columns (%d live: non-zero, not culled), %d quartets" % (name, L, n, live, nq))
        for label, ms, flop, nexp in (("tphip_unequal_quartet_tables_dev", ms_u, FLOP_UNEQUAL, EXPM1_UNEQUAL),
                                      ("tphip_quartet_tables_dev", ms_e, FLOP_EQUAL, EXPM1_EQUAL)):
            med = float(np.median(ms))
            tf = live_pairs * flop / (med * 1e-3) / 1e12
            print("  %-34s %10.3f ms (median of %d; min %.3f, max %.3f)" % (label, med, reps, min(ms), max(ms)))
            print("    %.3e (site, quartet) pairs/s over all columns, %.3e over the live ones; %d flop per live pair (source-counted, "
                  "expm1 not included) = %.2f TF = %.1f %% of the %.1f TF FP64 peak; %.2e expm1/s"
                  % (pairs / (med * 1e-3), live_pairs / (med * 1e-3), flop, tf, 100 * tf / PEAK_TF, PEAK_TF, nexp * live_pairs / (med * 1e-3)))
        print("  unequal / equal: time %.2f x, counted flop %.2f x, expm1 calls %.2f x"
              % (np.median(ms_u) / np.median(ms_e), FLOP_UNEQUAL / FLOP_EQUAL, EXPM1_UNEQUAL / EXPM1_EQUAL))
        got = urows.cpu().numpy()
        print("  locus 0, first and last quartet: p_correct %.4f %.4f, p_ac %.4f %.4f, p_ad %.4f %.4f"
              % (got[0, 0, 9], got[0, -1, 9], got[0, 0, 10], got[0, -1, 10], got[0, 0, 11], got[0, -1, 11]))
        plan.close()
        del d, rate, subst, lnl, flag, nres, tables, ws, urows, erows, uws, ews
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

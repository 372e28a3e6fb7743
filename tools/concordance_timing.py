"""Site concordance counts on a device-resident batch, after a warm-up:
  * tphip_concordance_counts_dev under HIP events on the column shapes of C2 (1000 loci x 500 columns) and C3 (100 loci x 50000
    columns), both with 64 taxa and the default sets of the 64-taxon tree the columns were simulated on (per internode the pooled
    set, the nearest-tip quartet and 100 quartets): median of `runs` calls, and set evaluations (set x column) per second;
  * a plain device-to-device copy of `states` on the same machine, the same way, and the ratio of the two times: how far the call
    is from reading the alignment once.
The call copies its set tables and waits for its kernels, so the events bracket what a caller pays.  No pass mark.
usage: python tools/concordance_timing.py [C3 | C2 ...] [runs=5] [quartets=100]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    import torch
    from tapir_amd import compute, engine, newick, synth
    pos = [a for a in sys.argv[1:] if "=" not in a] or ["C2", "C3"]
    opt = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
    runs, quartets = int(opt.get("runs", 5)), int(opt.get("quartets", 100))
    dev = torch.device("cuda")
    nt = 64
    for name in pos:
        L, n = synth.WORKLOADS[name][:2]
        seed = synth.WORKLOAD_SEED[name]
        tree = synth.yule_tree(nt, seed)
        d = synth.simulate(L, n, nt, seed, device=dev, tree=tree)
        names = [leaf.name for leaf in newick.leaves(d["root"])]
        rows = [d["names"].index(x) for x in names]                    # the sets name rows in leaf order
        states = d["states"][torch.tensor(rows, device=dev)].contiguous()
        groups = compute.tree_concordance_groups(d["root"])
        sets = compute.concordance_sets(groups, names, quartets=quartets)
        n_sets, ncols = int(sets["node_sets"][-1]), L * n
        single = int((np.diff(sets["group_offsets"][::4]) == 4).sum())
        d_off = torch.arange(L + 1, dtype=torch.int64, device=dev) * n
        d_counts = torch.empty((L, n_sets, 3), dtype=torch.int64, device=dev)
        copy = torch.empty_like(states)
        stream = torch.cuda.current_stream().cuda_stream
        call = lambda: engine.concordance_counts_dev(states, ncols, ncols, nt, d_off, L, sets["group_offsets"], sets["group_taxa"],  # noqa: E731
                                                     d_counts, stream=stream)
        call()                                                          # warm-up
        copy.copy_(states)
        torch.cuda.synchronize()
        ms, copy_ms = [], []
        for r in range(runs):
            a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            a.record()
            call()
            b.record()
            copy.copy_(states)
            c.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
            copy_ms.append(b.elapsed_time(c))
        med, cmed = float(np.median(ms)), float(np.median(copy_ms))
        total = d_counts.cpu().numpy().view(np.uint64).sum(axis=0)
        print("%s columns: %d loci x %d columns, %d taxa; %d internodes, %d sets (%d of four single taxa), %d taxa named"
              % (name, L, n, nt, len(groups), n_sets, single, len(sets["group_taxa"])))
        print("  tphip_concordance_counts_dev %10.3f ms (median of %d; min %.3f, max %.3f) = %.3e set evaluations/s, %.3e cells/s"
              % (med, runs, min(ms), max(ms), n_sets * ncols / (med * 1e-3), len(sets["group_taxa"]) * ncols / (med * 1e-3)))
        print("  copy of states (%.1f MB)      %10.3f ms (median of %d; min %.3f, max %.3f) = %.1f GB/s read + written; the call is %.0f x the copy"
              % (states.numel() / 1e6, cmed, runs, min(copy_ms), max(copy_ms), 2 * states.numel() / (cmed * 1e-3) / 1e9, med / cmed))
        print("  counts: %.3e decisive quartet sites in all (%.1f %% concordant)" % (float(total.sum()), 100.0 * float(total[:, 0].sum()) / max(1.0, float(total.sum()))))
        del d, states, copy, d_counts
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

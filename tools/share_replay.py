#!/usr/bin/env python3
"""CPU replay of how site_rate_kernel's persistent mode hands the work list out to its waves (no GPU needed).

  python tools/share_replay.py [--loci 6 --cols 2500 --taxa 64 --seed 5] [--waves 16 --grid-mult 3 --first-fraction 0.8]
                               [--window 128] [--plain-batch] [--reserve 0.15 --weights 2.9,2.04]

Every optimised column's number of likelihood evaluations comes from the CPU oracle (one call per column); the column's
`slow` mark is classify_kernel's rule (10 * Fitch changes >= 3 * (resolved taxa - 1)).  The replay then follows the kernel:
share boundaries (the `boundary` lambda), one segment per locus inside a share, 64 lanes, a free lane takes the next entry
of the segment, the segment ends with its last lane; a round is one evaluation issued for the whole wave.  It prints the
rounds summed over the waves in list order and with the marked columns moved to the front of every segment's last
`--window` entries (TPHIP_SITE_TAIL_ORDER, the default), and evaluations / (64 rounds) for both.

The default batch is the one tests/test_gpu_share_order.py runs (share_order_batch: an empty locus, a locus of constant
columns, a locus with fewer than 64 columns for the optimiser); --plain-batch takes synth.simulate's output as it is.

The hand-out by predicted work (TPHIP_SITE_SHARE_WORK=1) is replayed too: compact_kernel's reserve rule
(`reserve_split`: --reserve of every locus' unmarked columns, by their rank among them, form the locus' reserved tail), the
weighted scan (`class_prefixes`, --weights = predicted evaluations of a marked and of an unmarked column) and the share
boundaries (`work_shares`: the first `waves` shares cut the main parts into equal predicted work, the others the reserved
tails into equal column counts).  The last line printed compares the rounds of the two hand-outs and gives the mean
evaluations of the two classes, which is where the weights come from.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LANES = 64


def share_order_batch(nloci, ncols, ntaxa, seed):
    """The seeded batch of tests/test_gpu_share_order.py: synth.simulate(nloci, ncols, ntaxa, seed) with locus 2 emptied
    (locus 3 takes its columns), locus 0 overwritten with a constant column (no optimiser work) and locus 4 constant
    except for its first 40 columns (fewer optimiser columns than a wave has lanes).  Returns (states, offsets, d, pin)."""
    from tapir_amd import synth
    d = synth.simulate(nloci, ncols, ntaxa, seed)
    pin = synth.plan_inputs(d["root"], d["names"])
    st = d["states"].numpy().copy()
    off = d["locus_offsets"].copy()
    off[3] = off[2]
    st[:, off[0]:off[1]] = 1
    st[:, off[4] + 40:off[5]] = 2
    return np.ascontiguousarray(st), off, d, pin


def classify(states, parent, leaf):
    """classify_kernel's view of every column: (needs the optimiser, marked slow)."""
    from tapir_amd import eb
    m = states & 15
    m = np.where(m == 0, 15, m)
    res = m != 15
    resolved = res.sum(axis=0)
    uni = np.bitwise_or.reduce(np.where(res, m, 0), axis=0)
    popc = np.array([bin(x).count("1") for x in range(16)])[uni]
    optimised = (resolved > 1) & (popc != 1)
    changes = eb.parsimony_changes(states, parent, leaf)
    slow = 10 * changes >= 3 * np.maximum(resolved - 1, 1)
    return optimised, slow & optimised


def column_evals(states, off, pin, pi, exch, optimised):
    """Evaluations of every optimised column: the oracle called column by column (0 elsewhere)."""
    from oracle import oracle as orc
    ev = np.zeros(states.shape[1], dtype=np.int64)
    for l in range(len(off) - 1):
        for c in range(int(off[l]), int(off[l + 1])):
            if optimised[c]:
                ev[c] = orc.site_rates(states[:, c:c + 1], pin["parent"], pin["blen"], pin["leaf"], pi[l], exch[l])["nevals"]
    return ev


def boundary(b, total, first_round, nshares, first_fraction):
    """site_rate_kernel's share boundary b (the same double arithmetic)."""
    R, N = first_round, nshares
    if R >= N:
        return b * total // N
    f = first_fraction * b / R if b <= R else first_fraction + (1.0 - first_fraction) * (b - R) / (N - R)
    g = int(f * total)
    return total if b >= N else min(g, total)


RESERVE_SHIFT = 16   # site_rate_params.hpp: kReserveShift, kShareWeightShift
WEIGHT_SHIFT = 10


def fixed(x, shift):
    return int(round(x * (1 << shift)))


def reserved_before(r, q):
    """site_rate_params.hpp reserved_before: of the first r easy columns of a locus, how many are reserved (q = fraction * 2^16)."""
    return (np.asarray(r, dtype=np.int64) * int(q)) >> RESERVE_SHIFT


def reserve_split(slow, q):
    """compact_kernel's lists of one locus: `slow` is the mark of every work-list column in list order; returns the indices
    that stay in the main part and those that form the reserved tail (both in list order)."""
    slow = np.asarray(slow, dtype=bool)
    easy = ~slow
    rank = np.cumsum(easy) - easy          # easy columns before this one
    res = easy & (reserved_before(rank + 1, q) != reserved_before(rank, q))
    return np.flatnonzero(~res), np.flatnonzero(res)


def reserve_batch(slow, work_off, q):
    """compact_kernel's rule on a whole batch, as the kernel sees it: `slow` is the mark of every work-list column of the
    batch (loci concatenated), `work_off` the loci's offsets into it.  A column's rank counts the easy columns from the start
    of ITS locus.  Returns the mask of the reserved columns."""
    slow = np.asarray(slow, dtype=bool)
    easy = ~slow
    before = np.cumsum(easy) - easy                       # easy columns of the batch before this one
    work_off = np.asarray(work_off, dtype=np.int64)
    at_start = np.concatenate([[0], np.cumsum(easy)])[work_off[:-1]]
    rank = before - np.repeat(at_start, np.diff(work_off))
    return easy & (reserved_before(rank + 1, q) != reserved_before(rank, q))


def class_prefixes(n_slow, n_easy, q, w_slow, w_easy):
    """scan_counts_kernel: exclusive scans over the loci of (main-part columns, main-part predicted work, reserved-tail columns);
    the weights are fixed-point integers."""
    n_slow, n_easy = np.asarray(n_slow, dtype=np.int64), np.asarray(n_easy, dtype=np.int64)
    tail = reserved_before(n_easy, q)
    ex = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.int64)
    return ex(n_slow + n_easy - tail), ex(int(w_slow) * n_slow + int(w_easy) * (n_easy - tail)), ex(tail)


def work_shares(n_slow, n_easy, q, w_slow, w_easy, main_shares, nshares):
    """site_rate_kernel's shares by predicted work: for every share (in_tail, g0, g1), g0 / g1 counting columns of the
    concatenated main parts or of the concatenated reserved tails; also returns the two column prefixes."""
    mpre, wpre, tpre = class_prefixes(n_slow, n_easy, q, w_slow, w_easy)
    L = len(mpre) - 1
    wtotal, ttotal = int(wpre[-1]), int(tpre[-1])

    def main_cut(b):
        if b >= main_shares:
            return int(mpre[-1])
        target = b * wtotal // main_shares
        l, h = 0, L
        while h - l > 1:
            mid = (l + h) >> 1
            if wpre[mid] <= target:
                l = mid
            else:
                h = mid
        ww, nm = int(wpre[l + 1] - wpre[l]), int(mpre[l + 1] - mpre[l])
        return int(mpre[l]) + ((target - int(wpre[l])) * nm // ww if ww > 0 else 0)

    shares = []
    for b in range(nshares):
        if b >= main_shares:
            k, n = b - main_shares, nshares - main_shares
            shares.append((True, k * ttotal // n, (k + 1) * ttotal // n))
        else:
            shares.append((False, main_cut(b), main_cut(b + 1)))
    return shares, mpre, tpre


def replay_work(ev, slow, optimised, off, waves, grid_mult, reserve=0.15, weights=(2.9, 2.04), window=128, tail_order=True):
    """Rounds of one launch under the hand-out by predicted work (what Plan.last_round_count() reports)."""
    nshares = waves * grid_mult
    q = fixed(min(max(reserve, 0.0), 1.0), RESERVE_SHIFT) if grid_mult > 1 else 0
    main_shares = waves if q > 0 else nshares
    lists = [np.flatnonzero(optimised[int(off[l]):int(off[l + 1])]) + int(off[l]) for l in range(len(off) - 1)]
    parts = []
    for cols in lists:
        mi, ti = reserve_split(slow[cols], q)
        parts.append((cols[mi], cols[ti]))
    n_slow = [int(slow[c].sum()) for c in lists]
    n_easy = [len(c) - s for c, s in zip(lists, n_slow)]
    shares, mpre, tpre = work_shares(n_slow, n_easy, q, max(1, fixed(weights[0], WEIGHT_SHIFT)), max(1, fixed(weights[1], WEIGHT_SHIFT)),
                                     main_shares, nshares)
    rounds = 0
    for in_tail, g0, g1 in shares:
        pre = tpre if in_tail else mpre
        for l, pt in enumerate(parts):
            lo, hi = max(g0, int(pre[l])), min(g1, int(pre[l + 1]))
            if hi <= lo:
                continue
            seg = pt[1 if in_tail else 0][lo - int(pre[l]):hi - int(pre[l])]
            rounds += segment_rounds(tail_ordered(ev[seg], slow[seg], window) if tail_order else ev[seg])
    return rounds


def segment_rounds(ev):
    """Rounds one wave spends on a segment whose entries need ev[i] evaluations, taken in this order."""
    n = len(ev)
    left = np.zeros(LANES, dtype=np.int64)
    k = min(n, LANES)
    left[:k] = ev[:k]
    nxt, rounds = k, 0
    while True:
        rounds += 1
        left[left > 0] -= 1
        free = np.flatnonzero(left == 0)
        if nxt < n:
            take = min(len(free), n - nxt)
            left[free[:take]] = ev[nxt:nxt + take]
            nxt += take
        elif len(free) == LANES:
            return rounds


def tail_ordered(ev, slow, window):
    n = len(ev)
    wb = max(0, n - window)
    order = np.concatenate([np.arange(wb), wb + np.flatnonzero(slow[wb:]), wb + np.flatnonzero(~slow[wb:])])
    return ev[order]


def replay(ev, slow, optimised, off, waves, grid_mult, first_fraction, window=128):
    """(rounds in list order, rounds with the tail order, evaluations) of one launch."""
    lists = [np.flatnonzero(optimised[int(off[l]):int(off[l + 1])]) + int(off[l]) for l in range(len(off) - 1)]
    prefix = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    total = int(prefix[-1])
    nshares = waves * grid_mult
    plain = ordered = 0
    for b in range(nshares):
        g0 = boundary(b, total, waves, nshares, first_fraction)
        g1 = boundary(b + 1, total, waves, nshares, first_fraction)
        for l, cols in enumerate(lists):
            lo, hi = max(g0, int(prefix[l])), min(g1, int(prefix[l + 1]))
            if hi <= lo:
                continue
            seg = cols[lo - int(prefix[l]):hi - int(prefix[l])]
            plain += segment_rounds(ev[seg])
            ordered += segment_rounds(tail_ordered(ev[seg], slow[seg], window))
    return plain, ordered, int(ev.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=6)
    ap.add_argument("--cols", type=int, default=2500)
    ap.add_argument("--taxa", type=int, default=64)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--waves", type=int, default=16)
    ap.add_argument("--grid-mult", type=int, default=3)
    ap.add_argument("--first-fraction", type=float, default=0.8)
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--plain-batch", action="store_true")
    ap.add_argument("--reserve", type=float, default=0.15)
    ap.add_argument("--weights", default="2.9,2.04")
    a = ap.parse_args()
    if a.plain_batch:
        from tapir_amd import synth
        d = synth.simulate(a.loci, a.cols, a.taxa, a.seed)
        pin = synth.plan_inputs(d["root"], d["names"])
        st, off = d["states"].numpy(), d["locus_offsets"]
    else:
        st, off, d, pin = share_order_batch(a.loci, a.cols, a.taxa, a.seed)
    optimised, slow = classify(st, pin["parent"], pin["leaf"])
    ev = column_evals(st, off, pin, d["pi"], d["exch"], optimised)
    plain, ordered, evals = replay(ev, slow, optimised, off, a.waves, a.grid_mult, a.first_fraction, a.window)
    hist = np.bincount(ev[optimised], minlength=8)
    print("columns for the optimiser %d (marked slow %d), evaluations %d, per column %.3f; histogram of evaluations %s"
          % (optimised.sum(), slow.sum(), evals, evals / max(1, optimised.sum()), hist.tolist()))
    print("mean evaluations: marked %.3f, unmarked %.3f" % (ev[slow].mean() if slow.any() else 0.0,
                                                           ev[optimised & ~slow].mean() if (optimised & ~slow).any() else 0.0))
    print("rounds in list order %d (lane use %.4f), with the last %d entries of every segment ordered %d (lane use %.4f): %.2f %% fewer"
          % (plain, evals / (64.0 * plain), a.window, ordered, evals / (64.0 * ordered), 100.0 * (plain - ordered) / plain))
    weights = tuple(float(x) for x in a.weights.split(","))
    new = replay_work(ev, slow, optimised, off, a.waves, a.grid_mult, a.reserve, weights, a.window)
    print("shares by predicted work (reserve %.3f, weights %s): %d rounds (lane use %.4f) against %d: %.2f %% fewer"
          % (a.reserve, a.weights, new, evals / (64.0 * new), ordered, 100.0 * (ordered - new) / ordered))


if __name__ == "__main__":
    main()

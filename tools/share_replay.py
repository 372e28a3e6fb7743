#!/usr/bin/env python3
"""CPU replay of how site_rate_kernel's persistent mode hands the work list out to its waves (no GPU needed).

  python tools/share_replay.py [--loci 6 --cols 2500 --taxa 64 --seed 5] [--waves 16 --grid-mult 3 --first-fraction 0.8]
                               [--window 128] [--plain-batch] [--reserve 0.15 --weights 2.9,2.04]
                               [--tail-shares big,mid,small[,frac_big,frac_mid] | auto | 0] [--align-loci]

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
tails).  The later shares cut the tails into equal column counts (--tail-shares 0, the default here and the library's own for
batches whose later shares come from the knobs alone) or in whole lane-fills, long shares first (tail_shares.hpp:
--tail-shares 8,4,2 or auto = what decide_site_launch takes for a batch of this size).  The last lines printed compare the
rounds of the two hand-outs, give the mean evaluations of the two classes, which is where the weights come from, and the
makespan: the shares dealt in grid order to whichever of the --waves slots is free first, the round at which the last slot
finishes and the spread between the slots.
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


# launch_constants.hpp: kTailFillsBig / Mid / Small, kTailFracBig / Mid
DEFAULT_TAIL_FILLS = (5, 3, 2)
DEFAULT_TAIL_FRACS = (0.4, 0.3)


def tail_shares(big, mid, small, frac_big=DEFAULT_TAIL_FRACS[0], frac_mid=DEFAULT_TAIL_FRACS[1]):
    """decide_site_launch's TailShares (tail_shares.hpp) from a knob's numbers: (fills_big, fills_mid, fills_small, frac_big_q,
    frac_mid_q) with big >= mid >= small >= 1 and the fractions in units of 2^-16; big = 0: None (equal column counts)."""
    if big <= 0:
        return None
    small = max(1, min(small, 1 << 20))
    mid = max(small, min(mid, 1 << 20))
    big = max(mid, min(big, 1 << 20))
    fb = min(max(frac_big, 0.0), 1.0)
    fm = min(max(frac_mid, 0.0), 1.0 - fb)
    fbq = fixed(fb, RESERVE_SHIFT)
    return big, mid, small, fbq, min(fixed(fm, RESERVE_SHIFT), (1 << RESERVE_SHIFT) - fbq)


def parse_tail_shares(text):
    """TPHIP_SITE_TAIL_SHARES: "big,mid,small[,frac_big,frac_mid]", or "0" for equal column counts."""
    v = text.split(",")
    if len(v) == 1 and int(v[0]) == 0:
        return None
    if len(v) == 3:
        return tail_shares(int(v[0]), int(v[1]), int(v[2]))
    if len(v) == 5:
        return tail_shares(int(v[0]), int(v[1]), int(v[2]), float(v[3]), float(v[4]))
    raise ValueError("tail shares: big,mid,small[,frac_big,frac_mid] or 0")


def tail_bands(ttotal, ts):
    """tail_shares.hpp tail_bands: (fills, edge1, edge2, n1, n2, n3)."""
    big, mid, small, fbq, fmq = ts[:5]
    fills = (ttotal + LANES - 1) // LANES
    n1 = ((fills * fbq) >> RESERVE_SHIFT) // big
    n2 = ((fills * fmq) >> RESERVE_SHIFT) // mid
    e1 = n1 * big
    e2 = e1 + n2 * mid
    return fills, e1, e2, n1, n2, (fills - e2 + small - 1) // small


def tail_share_range(k, ttotal, ts):
    """tail_shares.hpp tail_share_range: columns [g0, g1) of the k-th later share; (0, 0) past the last share needed."""
    big, mid, small = ts[:3]
    _, e1, e2, n1, n2, n3 = tail_bands(ttotal, ts)
    if k < n1:
        f0, f1 = k * big, (k + 1) * big
    elif k < n1 + n2:
        f0 = e1 + (k - n1) * mid
        f1 = f0 + mid
    elif k < n1 + n2 + n3:
        f0 = e2 + (k - n1 - n2) * small
        f1 = f0 + small
    else:
        return 0, 0
    return f0 * LANES, min(f1 * LANES, ttotal)


def tail_share_count(ttotal, ts):
    return sum(tail_bands(ttotal, ts)[3:])


def tail_share_bound(ttotal_max, ts):
    """tail_shares.hpp tail_share_bound: at least tail_share_count(t) for every t <= ttotal_max."""
    big, mid, small, fbq, fmq = ts[:5]
    F = (ttotal_max + LANES - 1) // LANES
    rest = F - ((F * (fbq + fmq)) >> RESERVE_SHIFT) + big + mid - 1
    return ((F * fbq) >> RESERVE_SHIFT) // big + ((F * fmq) >> RESERVE_SHIFT) // mid + (min(rest, F) + small - 1) // small


def default_tail_shares(ncols, waves, grid_mult, q):
    """decide_site_launch without TPHIP_SITE_TAIL_SHARES: batches whose equal share is at least 1500 columns cut the tails in
    whole lane-fills, the default fills times the smallest factor with which the longest possible tails fit the grid, where the
    tails hold at least a fill per later workgroup (a sixth entry: TailShares::min_total); the others (later shares by the
    knobs alone) keep equal column counts: None."""
    if q <= 0 or grid_mult <= 1 or ncols // max(1, waves) < 1500:
        return None
    tails_max = (ncols * q) >> RESERVE_SHIFT
    scale = 1
    while True:
        ts = tail_shares(*(f * scale for f in DEFAULT_TAIL_FILLS))
        if tail_share_bound(tails_max, ts) <= waves * (grid_mult - 1) or scale >= 1 << 16:
            return ts + (min(LANES * waves * (grid_mult - 1), (1 << 31) - 1),)
        scale += 1


def work_shares(n_slow, n_easy, q, w_slow, w_easy, main_shares, nshares, tail=None, align_loci=False):
    """site_rate_kernel's shares by predicted work: for every share (in_tail, g0, g1), g0 / g1 counting columns of the
    concatenated main parts or of the concatenated reserved tails; also returns the two column prefixes.  `tail`: the
    TailShares of the later shares (tail_shares()), None = equal column counts over the nshares - main_shares of them; with it
    the list ends with the last share that the tails need.  align_loci (an experiment that the kernel does not have): every
    locus' tail begins a fresh lane-fill, g0 / g1 and the returned tail prefix then count the padded tails."""
    mpre, wpre, tpre = class_prefixes(n_slow, n_easy, q, w_slow, w_easy)
    if align_loci:
        tpre = np.concatenate([[0], np.cumsum((np.diff(tpre) + LANES - 1) // LANES * LANES)]).astype(np.int64)
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
    if tail is not None and len(tail) > 5 and ttotal < tail[5]:     # tail_shares_apply
        tail = None
    if tail is not None and main_shares < nshares:
        nshares = main_shares + tail_share_count(ttotal, tail)
    for b in range(nshares):
        if b >= main_shares and tail is not None:
            shares.append((True,) + tail_share_range(b - main_shares, ttotal, tail))
        elif b >= main_shares:
            k, n = b - main_shares, nshares - main_shares
            shares.append((True, k * ttotal // n, (k + 1) * ttotal // n))
        else:
            shares.append((False, main_cut(b), main_cut(b + 1)))
    return shares, mpre, tpre


def share_rounds_work(ev, slow, optimised, off, waves, grid_mult, reserve=0.15, weights=(2.9, 2.04), window=128, tail_order=True,
                      tail=None, align_loci=False):
    """Rounds of every share, in grid order, of one launch under the hand-out by predicted work.  `tail`: the later shares'
    TailShares (tail_shares(), parse_tail_shares(), default_tail_shares()); None = equal column counts, which is what the
    library does for a batch whose later shares come from the knobs alone (default_tail_shares)."""
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
                                     main_shares, nshares, tail if q > 0 else None, align_loci)
    out = []
    for in_tail, g0, g1 in shares:
        pre = tpre if in_tail else mpre
        rounds = 0
        for l, pt in enumerate(parts):
            mine = pt[1 if in_tail else 0]
            lo, hi = max(g0, int(pre[l])), min(g1, int(pre[l]) + len(mine))   # (aligned tails: the padding holds no column)
            if hi <= lo:
                continue
            seg = mine[lo - int(pre[l]):hi - int(pre[l])]
            rounds += segment_rounds(tail_ordered(ev[seg], slow[seg], window) if tail_order else ev[seg])
        out.append(rounds)
    return out


def replay_work(ev, slow, optimised, off, waves, grid_mult, reserve=0.15, weights=(2.9, 2.04), window=128, tail_order=True, tail=None):
    """Rounds of one launch under the hand-out by predicted work (what Plan.last_round_count() reports)."""
    return sum(share_rounds_work(ev, slow, optimised, off, waves, grid_mult, reserve, weights, window, tail_order, tail))


def makespan(share_rounds, waves):
    """The shares, in grid order, each to whichever of the `waves` slots is free first (what the dispatcher does with the
    workgroups of a grid larger than the resident waves), a round costing every wave the same time: (the round at which the
    last slot finishes, the spread between the first and the last slot to finish).  The rounds' sum cannot see what short
    last shares are for; this can."""
    import heapq
    slots = [0] * waves
    heapq.heapify(slots)
    for r in share_rounds:
        if r > 0:    # a workgroup without columns leaves at once
            heapq.heappush(slots, heapq.heappop(slots) + r)
    return max(slots), max(slots) - min(slots)


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
    ap.add_argument("--tail-shares", default="0")
    ap.add_argument("--align-loci", action="store_true")
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
    q = fixed(min(max(a.reserve, 0.0), 1.0), RESERVE_SHIFT) if a.grid_mult > 1 else 0
    tail = default_tail_shares(st.shape[1], a.waves, a.grid_mult, q) if a.tail_shares == "auto" else parse_tail_shares(a.tail_shares)
    per_share = share_rounds_work(ev, slow, optimised, off, a.waves, a.grid_mult, a.reserve, weights, a.window, True, tail, a.align_loci)
    new = sum(per_share)
    print("shares by predicted work (reserve %.3f, weights %s): %d rounds (lane use %.4f) against %d: %.2f %% fewer"
          % (a.reserve, a.weights, new, evals / (64.0 * new), ordered, 100.0 * (ordered - new) / ordered))
    last, spread = makespan(per_share, a.waves)
    print("later shares %s: %d shares with columns, the last of %d slots finishes at round %d (ideal %.1f), spread between the slots %d"
          % ("of equal column counts" if tail is None else "of %d/%d/%d lane-fills (fractions %.3f, %.3f)%s"
             % (tail[0], tail[1], tail[2], tail[3] / 65536.0, tail[4] / 65536.0, ", aligned per locus" if a.align_loci else ""),
             sum(r > 0 for r in per_share), a.waves, last, evals / (64.0 * a.waves), spread))


if __name__ == "__main__":
    main()

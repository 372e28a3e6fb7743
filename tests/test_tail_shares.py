"""The later shares' cut of the reserved tails on the CPU: tapir_amd/csrc/tail_shares.hpp (and site_launch_plan.hpp's use of it)
compiled with g++ into tests/native/tail_shares_dump.cpp, against a restatement that walks the fills one share at a time
(`restated`, below: a loop where the header has a closed form) and against tools/share_replay.py's copy of the arithmetic."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import share_replay as rp  # noqa: E402

HALF, QUARTER = 32768, 16384
# (big, mid, small, frac_big_q, frac_mid_q): equal fills, the two tapers of the issue, single fills, other fractions
GEOMETRIES = [(3, 3, 3, HALF, QUARTER), (8, 4, 2, HALF, QUARTER), (6, 3, 1, HALF, QUARTER), (1, 1, 1, HALF, QUARTER),
              (8, 4, 2, QUARTER, QUARTER), (4, 2, 1, 0, 0), (5, 2, 2, 65536, 0)]


def totals(big):
    """Tails' lengths: around one and two fills, one short of a big share, and around the lengths at which a band's edge
    falls exactly on a fill (half of 2 n big fills is n big shares exactly; a fill more or less is one past / one short)."""
    t = [0, 1, 63, 64, 65, 127, 128, 129, 64 * big - 1, 64 * big, 64 * big + 1]
    for fills in (2 * big, 4 * big, 4 * big * 3, 64 * big):
        for f in (fills - 1, fills, fills + 1):
            t += [64 * f - 1, 64 * f, 64 * f + 1]
    return sorted(set(x for x in t + [64 * 1000 + 17, 749900] if x >= 0))


def restated(ttotal, geom):
    """The shares' column ranges, one share after the other."""
    big, mid, small, fbq, fmq = geom
    fills = -(-ttotal // 64)
    out, f = [], 0
    for size, share in ((big, fills * fbq // 65536), (mid, fills * fmq // 65536)):
        for _ in range(share // size):
            out.append((f, f + size))
            f += size
    while f < fills:
        out.append((f, min(f + small, fills)))
        f += small
    return [(64 * a, min(64 * b, ttotal)) for a, b in out]


def build_dump(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "tail_shares_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "tapir_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "tail_shares_dump.cpp"), "-o", exe])
    return exe


def ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    assert out.stderr == ""
    return [[int(x) for x in ln.split()[1:]] for ln in out.stdout.splitlines()]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("tail_shares"))


def range_lines():
    lines, keys = [], []
    for g in GEOMETRIES:
        for t in totals(g[0]):
            kmax = len(restated(t, g)) + 70      # past the last share needed and past the host's bound (checked below)
            lines.append("ranges %d %d %d %d %d %d %d" % (g + (t, kmax)))
            keys.append((g, t, kmax))
    return lines, keys


def check_ranges(answers, keys):
    for (g, t, kmax), a in zip(keys, answers):
        count, bound, flat = a[0], a[1], a[2:]
        got = list(zip(flat[0::2], flat[1::2]))
        want = restated(t, g)
        assert len(got) == kmax and count == len(want) and bound >= count and kmax > bound, (g, t)
        assert got[:count] == want, (g, t)
        assert all(r == (0, 0) for r in got[count:]), (g, t)          # every k past the last needed share is empty
        # the ranges tile [0, t) in order; every cut but the last is a multiple of 64; lengths never increase
        at = 0
        for g0, g1 in got[:count]:
            assert g0 == at and g1 > g0 and g0 % 64 == 0, (g, t)
            at = g1
        assert at == t and all(g1 % 64 == 0 for _, g1 in got[:count - 1]), (g, t)
        lens = [g1 - g0 for g0, g1 in got[:count]]
        assert all(a >= b for a, b in zip(lens, lens[1:])), (g, t)
        # the replay's copy of the arithmetic
        assert [rp.tail_share_range(k, t, g) for k in range(kmax)] == got and rp.tail_share_count(t, g) == count, (g, t)
        assert rp.tail_share_bound(t, g) == bound


def test_ranges_tile_the_tails(exe):
    lines, keys = range_lines()
    check_ranges(ask(exe, lines), keys)


def test_bound_covers_every_shorter_tail(exe):
    """tail_share_bound(T) is at least the shares of every t <= T (the count itself goes down where a fill more turns short
    shares into a long one), and never decreases with T."""
    for g in GEOMETRIES:
        tmax = 64 * 20 * g[0] + 5
        bounds = [b[0] for b in ask(exe, ["bound %d %d %d %d %d %d" % (g + (t,)) for t in range(tmax + 1)])]
        most = 0
        for t in range(tmax + 1):
            most = max(most, len(restated(t, g)))
            assert bounds[t] >= most, (g, t)
        assert all(a <= b for a, b in zip(bounds, bounds[1:])), g


def reserved(r, q):
    return (r * q) >> 16


DECIDE = "decide %d %d %d %d %d %d %d %s"
FIELDS = ("waves", "grid_mult", "share_work", "reserve_q", "big", "mid", "small", "fbq", "fmq", "bound", "grid", "spill", "min_total")


def decide(exe, ntaxa, nwords, depth, nloci, cols, cus, per_cu, **knobs):
    text = " ".join("%s=%s" % kv for kv in knobs.items())
    return dict(zip(FIELDS, ask(exe, [DECIDE % (ntaxa, nwords, depth, nloci, cols, cus, per_cu, text)])[0]))


def test_default_geometry_and_the_parents_grid(exe):
    """bench.py's C3 shape (case A of test_site_launch.py): the default fills, the parent's grid of waves x 3.  With every easy
    column reserved the fills grow until the longest tails fit that grid.  A batch that has later shares by the knobs alone
    (test_gpu_share_work.py's) keeps equal column counts, and so does TPHIP_SITE_TAIL_SHARES=0 everywhere."""
    a = decide(exe, 64, 8, 3, 100, 50000, 256, 8)
    assert (a["waves"], a["grid_mult"], a["share_work"], a["reserve_q"]) == (2048, 3, 1, 9830)
    assert (a["big"], a["mid"], a["small"]) == rp.DEFAULT_TAIL_FILLS == (5, 3, 2)
    assert (a["fbq"], a["fmq"]) == (26214, 19661) == tuple(rp.fixed(f, 16) for f in rp.DEFAULT_TAIL_FRACS)
    assert a["grid"] == 6144 and 0 < a["bound"] <= 4096
    assert a["min_total"] == 64 * 4096        # tails of less than a fill per later workgroup keep the equal column counts
    assert rp.default_tail_shares(5000000, 2048, 3, 9830) == (5, 3, 2, 26214, 19661, 64 * 4096)
    m = decide(exe, 64, 8, 3, 100, 50000, 256, 8, TPHIP_SITE_RESERVE="1.0")
    assert m["grid"] == 6144 and m["bound"] <= 4096 and 2 * m["big"] == 5 * m["small"] and 2 * m["mid"] == 3 * m["small"] and m["small"] > 2
    assert rp.default_tail_shares(5000000, 2048, 3, 65536) == (m["big"], m["mid"], m["small"], 26214, 19661, 64 * 4096)
    off = decide(exe, 64, 8, 3, 100, 50000, 256, 8, TPHIP_SITE_TAIL_SHARES="0")
    assert (off["big"], off["bound"], off["grid"]) == (0, 0, 6144)
    h = dict(TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_WAVES="16", TPHIP_SITE_GRID_MULT="3", TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0.25")
    s = decide(exe, 64, 8, 3, 6, 2500, 256, 8, **h)
    assert (s["share_work"], s["reserve_q"], s["big"], s["bound"], s["grid"]) == (1, 16384, 0, 0, 48)
    assert rp.default_tail_shares(15000, 16, 3, 16384) is None
    s = decide(exe, 64, 8, 3, 6, 2500, 256, 8, TPHIP_SITE_TAIL_SHARES="1,1,1", **h)     # 3750 columns at most: 59 single fills
    assert (s["big"], s["mid"], s["small"], s["fbq"], s["fmq"], s["min_total"]) == (1, 1, 1, 26214, 19661, 0) and s["grid"] == 16 + s["bound"] >= 16 + 59
    s = decide(exe, 64, 8, 3, 6, 2500, 256, 8, TPHIP_SITE_TAIL_SHARES="2,4,8,0.3,0.9", **h)   # out of order: big >= mid >= small
    assert (s["big"], s["mid"], s["small"], s["fbq"], s["fmq"]) == (8, 8, 8, rp.fixed(0.3, 16), 65536 - rp.fixed(0.3, 16))
    assert rp.parse_tail_shares("2,4,8,0.3,0.9") == (8, 8, 8, s["fbq"], s["fmq"])
    s = decide(exe, 64, 8, 3, 6, 2500, 256, 8, TPHIP_SITE_TAIL_SHARES="nonsense", **h)        # text that does not parse: not set
    assert (s["big"], s["grid"]) == (0, 48)


def test_grid_holds_every_split_of_the_tails(exe):
    """The host's grid against the shares that any batch of the shape can need: per-locus tails reserved_before(easy columns,
    reserve) for easy-column counts up to the locus' length, drawn at random and at the extremes."""
    rng = np.random.default_rng(17)
    shapes = [dict(nloci=5, cols=20000, knobs={}),
              dict(nloci=5, cols=20000, knobs=dict(TPHIP_SITE_RESERVE="0.31")),
              dict(nloci=5, cols=20000, knobs=dict(TPHIP_SITE_RESERVE="1.0")),
              dict(nloci=7, cols=9001, knobs=dict(TPHIP_SITE_TAIL_SHARES="1,1,1")),
              dict(nloci=7, cols=9001, knobs=dict(TPHIP_SITE_TAIL_SHARES="6,3,1,0.4,0.4", TPHIP_SITE_RESERVE="0.5")),
              dict(nloci=3, cols=700, knobs=dict(TPHIP_SITE_TAIL_SHARES="2,2,2", TPHIP_SITE_PERSISTENT="1", TPHIP_SITE_GRID_MULT="3",
                                                 TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0.25"))]
    for sh in shapes:
        d = decide(exe, 64, 8, 3, sh["nloci"], sh["cols"], 4, 4, **sh["knobs"])
        assert d["waves"] == 16 and d["share_work"] == 1 and d["big"] > 0, sh
        geom = (d["big"], d["mid"], d["small"], d["fbq"], d["fmq"])
        assert d["grid"] >= d["waves"] * d["grid_mult"] and d["grid"] >= d["waves"] + d["bound"], sh
        if "TPHIP_SITE_TAIL_SHARES" not in sh["knobs"]:
            assert d["grid"] == d["waves"] * d["grid_mult"], sh          # the default fills fit the parent's grid
        splits = [np.full(sh["nloci"], sh["cols"]), np.zeros(sh["nloci"], dtype=np.int64)]
        splits += [rng.integers(0, sh["cols"] + 1, sh["nloci"]) for _ in range(200)]
        splits += [np.where(rng.random(sh["nloci"]) < 0.5, sh["cols"], rng.integers(0, 70, sh["nloci"])) for _ in range(50)]
        for easy in splits:
            ttotal = sum(reserved(int(e), d["reserve_q"]) for e in easy)
            assert len(restated(ttotal, geom)) <= d["grid"] - d["waves"], (sh, easy)


def test_spill_rows_cover_the_grid(exe):
    """The spilled-stack variant keeps one scratch row per workgroup (indexed by blockIdx.x): the rows follow the grid."""
    # 256 taxa, 21 loci x 100 000 columns: 8 x 256 waves with the fourth parked partial spilled (1025 columns per wave: the
    # later shares come from the knobs)
    knobs = dict(TPHIP_SITE_GRID_MULT="3", TPHIP_SITE_SHARE_WORK="1", TPHIP_SITE_RESERVE="0.25")
    row = 12 * 64 * 8
    d = decide(exe, 256, 32, 4, 21, 100000, 256, 6, **knobs)
    assert (d["waves"], d["big"], d["grid"], d["spill"]) == (2048, 0, 6144, 6144 * row)
    d = decide(exe, 256, 32, 4, 21, 100000, 256, 6, TPHIP_SITE_TAIL_SHARES="8,4,2", **knobs)
    assert (d["big"], d["grid"], d["spill"]) == (8, 6144, 6144 * row) and d["bound"] <= 4096      # 525 000 columns at most: 8204 fills
    d = decide(exe, 256, 32, 4, 21, 100000, 256, 6, TPHIP_SITE_TAIL_SHARES="1,1,1", **knobs)
    assert d["grid"] == 2048 + d["bound"] >= 2048 + 8204 and d["spill"] == d["grid"] * row


def test_sanitized_dump(tmp_path):
    """The same cases through a build with the address and undefined-behaviour sanitizers (a stand-alone program)."""
    exe = build_dump(tmp_path, extra=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    lines, keys = range_lines()
    check_ranges(ask(exe, lines), keys)
    g = GEOMETRIES[1]
    ask(exe, ["bound %d %d %d %d %d %d" % (g + (t,)) for t in (0, 1, 64, 749900, 1 << 40)])
    ask(exe, [DECIDE % (64, 8, 3, 100, 50000, 256, 8, ""), DECIDE % (64, 8, 3, 100, 50000, 256, 8, "TPHIP_SITE_RESERVE=1.0"),
              DECIDE % (256, 32, 4, 21, 100000, 256, 6, "TPHIP_SITE_GRID_MULT=3 TPHIP_SITE_SHARE_WORK=1 TPHIP_SITE_RESERVE=0.25 "
                        "TPHIP_SITE_TAIL_SHARES=1,1,1")])

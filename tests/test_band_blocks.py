"""How the replicate-band stages (site bootstrap, parametric bootstrap, posterior PI) cut their work to the caller's workspace,
decided on the CPU: tapir_amd/csrc/band_blocks.hpp compiled with g++ into tests/native/band_blocks_dump.cpp, which walks a
workspace block by block the way the drivers do.  Every region starts on a multiple of 256 bytes; the site bootstrap keeps per
block the per-site integrals [columns][n_i] of doubles, the counts [replicates][columns rounded up to even] of 16-bit counters and
the rows [loci][B][Wb] of doubles after a fixed part of 256 bytes and the stream ids; a block is as many consecutive loci as fit
with all B replicates (65535 at most), and a locus that does not fit alone draws its replicates in whole tiles of 128.  The
expected values are restated here from those rules, not read from the header."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tapir_amd", "csrc")
TILE, CAP, MAX_LOCI = 128, 1 << 30, 65535

# sizes, T, n_i, B: min, preferred, blocks (l0, l1, range) at min, blocks at preferred
PINNED = [
    ([50, 7, 0, 300], 10, 1, 130, 91392, 142592, [(0, 3, 130), (3, 4, 128)], [(0, 4, 130)]),
    ([50, 7, 0, 300], 10, 1, 300, 106496, 324352, [(0, 2, 300), (2, 3, 300), (3, 4, 128)], [(0, 4, 300)]),
    ([1025, 64, 65], 8, 2, 2, 21760, 24576, [(0, 1, 2), (1, 3, 2)], [(0, 3, 2)]),
    ([10], 5, 0, 10, 1280, 1280, [(0, 1, 10)], [(0, 1, 10)]),
]


def au(x):
    return (x + 255) // 256 * 256


def integ(cols, n_i):
    return au(8 * cols * n_i)


def counts(cols, reps):
    return au(2 * ((cols + 1) // 2 * 2) * reps)


def rows(loci, B, Wb):
    return au(8 * loci * B * Wb)


def bs_block(cols, loci, reps, B, n_i, Wb):
    return integ(cols, n_i) + counts(cols, reps) + rows(loci, B, Wb)


def bs_sizes(sizes, T, n_i, B):
    """(fixed, one, all) of the site bootstrap."""
    Wb = T + n_i
    one = max([bs_block(n, 1, min(B, TILE), B, n_i, Wb) for n in sizes], default=0)
    return 256 + au(8 * len(sizes)), one, bs_block(sum(sizes), len(sizes), B, B, n_i, Wb)


def pp_block(loci, K, B, Wb):
    return au(8 * loci * K * Wb) + au(4 * loci * B * K) + rows(loci, B, Wb)


def build_dump(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "band_blocks_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "band_blocks_dump.cpp"), "-o", exe])
    return exe


def run_dump(exe, queries):
    text = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, check=True).stdout
    got = [[int(v) for v in line.split()] for line in text.splitlines()]
    assert len(got) == len(queries)
    return got


def bs_query(at, d, sizes, T, n_i, B):
    return "bs %d %d %d %d %d %d %d %s" % (at, d, TILE, T, n_i, B, len(sizes), " ".join(map(str, sizes)))


def bs_answer(row):
    mn, pf, usable, nb = row[:4]
    return mn, pf, usable, [tuple(row[4 + 3 * k:7 + 3 * k]) for k in range(nb)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("band_blocks"))


def pinned_queries():
    q = []
    for sizes, T, n_i, B, *_ in PINNED:
        q += [bs_query(4096, 0, sizes, T, n_i, B), bs_query(4096, -1, sizes, T, n_i, B), bs_query(4096 + 1, 255, sizes, T, n_i, B)]
    return q


def check_pinned(got):
    for k, (sizes, T, n_i, B, mn, pf, at_min, at_pf) in enumerate(PINNED):
        a, b, c = (bs_answer(r) for r in got[3 * k:3 * k + 3])
        print(sizes, T, n_i, B, "min", a[0], "preferred", a[1], "at min", a[3], "at preferred", b[3], "1 off with min + 255", c[3])
        assert (a[0], a[1]) == (mn, pf) == (b[0], b[1])
        assert a[3] == at_min and b[3] == at_pf
        assert c[3] == at_min and c[2] == a[2]          # a pointer misaligned by 1 with min + 255 bytes: the blocks of min


def test_pinned_blocks(exe):
    check_pinned(run_dump(exe, pinned_queries()))


def test_pinned_sizes_follow_from_the_rules():
    """The table's sizes are what the rules at the top give: no figure is taken from the code under test."""
    for sizes, T, n_i, B, mn, pf, _, _ in PINNED:
        fixed, one, every = bs_sizes(sizes, T, n_i, B)
        assert (fixed + one, fixed + max(one, min(every, CAP))) == (mn, pf)


def test_base_and_usable(exe):
    got = run_dump(exe, ["base 4096 1000", "base 4097 1000", "base 4097 255", "base 4097 254", "base 4351 10", "base 4351 0", "base 4352 0"])
    assert got == [[4096, 1000], [4352, 745], [4352, 0], [4352, 0], [4352, 9], [4352, 0], [4352, 0]]   # 0, never a wrapped number


def test_a_block_holds_65535_loci_at_most(exe):
    sizes = [1] * 70000
    mn, pf, usable, blocks = bs_answer(run_dump(exe, [bs_query(4096, -1, sizes, 1, 0, 2)])[0])
    assert bs_block(70000, 70000, 2, 2, 0, 1) <= usable and blocks == [(0, 65535, 2), (65535, 70000, 2)]
    assert run_dump(exe, ["pp 4096 -1 1 2 2 70000"])[0][3] == 65535


def check_bs_blocks(sizes, T, n_i, B, usable, blocks):
    L, Wb = len(sizes), T + n_i
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    at = 0
    for l0, l1, rng in blocks:
        assert l0 == at and l0 < l1 <= L and l1 - l0 <= MAX_LOCI
        at = l1
        n = off[l1] - off[l0]
        if bs_block(n, l1 - l0, B, B, n_i, Wb) <= usable:      # all B replicates' counts fit: the loci go together
            assert rng == B
            assert l1 == L or l1 - l0 == MAX_LOCI or bs_block(off[l1 + 1] - off[l0], l1 + 1 - l0, B, B, n_i, Wb) > usable
        else:                                                  # a lone long locus, in ranges of whole tiles
            assert l1 == l0 + 1 and rng % TILE == 0 and 0 < rng < B
            assert bs_block(n, 1, rng, B, n_i, Wb) <= usable
            assert rng + TILE > B or bs_block(n, 1, rng + TILE, B, n_i, Wb) > usable
    assert at == L


def test_bootstrap_blocks_over_a_sweep(exe):
    rnd = random.Random(20240611)
    cases, queries = [], []
    for _ in range(600):
        sizes = [rnd.choice([0, 1, 2, 63, 64, 65, rnd.randrange(3001), rnd.randrange(3001)]) for _ in range(rnd.randrange(1, 8))]
        T, n_i, B = rnd.randrange(1, 13), rnd.randrange(4), rnd.choice([2, 3, 127, 128, 129, 300, 4096])
        at = 4096 + rnd.choice([0, 0, 1, 8, 255])
        for d in (0, 1, 2, 255, 256, 257, 4096, 65536, -1):
            cases.append((sizes, T, n_i, B, at, d))
            queries.append(bs_query(at, d, sizes, T, n_i, B))
    lone = 0
    for (sizes, T, n_i, B, at, d), row in zip(cases, run_dump(exe, queries)):
        mn, pf, usable, blocks = bs_answer(row)
        fixed, one, every = bs_sizes(sizes, T, n_i, B)
        assert mn == fixed + one and pf == fixed + max(one, min(every, CAP)) and mn <= pf <= fixed + max(one, CAP)
        pad = -at % 256
        ws = pf if d < 0 else mn + d
        assert usable == max(ws - pad, 0) - au(8 * len(sizes))
        assert usable >= one          # at ws = min too: the fixed part allows for aligning the pointer up
        check_bs_blocks(sizes, T, n_i, B, usable, blocks)
        lone += sum(1 for b in blocks if b[2] != B)
        if d < 0 and pad == 0 and every <= CAP:
            assert blocks == [(0, len(sizes), B)]
    print("%d walks, %d lone-locus blocks in ranges" % (len(cases), lone))
    assert lone > 100


def test_resample_blocks_over_a_sweep(exe):
    rnd = random.Random(7)
    cases, queries = [], []
    for _ in range(300):
        sizes = [rnd.choice([0, 1, 31, 32, 33, rnd.randrange(3001)]) for _ in range(rnd.randrange(1, 8))]
        n_i = rnd.randrange(4)
        for d in (0, 1, 256, 4096, -1):
            cases.append((sizes, n_i, d))
            queries.append("rs 4096 %d %d %d %s" % (d, n_i, len(sizes), " ".join(map(str, sizes))))
    for (sizes, n_i, d), row in zip(cases, run_dump(exe, queries)):
        mn, pf, usable, nb = row[:4]
        blocks = [tuple(row[4 + 2 * k:6 + 2 * k]) for k in range(nb)]
        one, every = integ(max(sizes), n_i), integ(sum(sizes), n_i)
        assert (mn, pf) == (256 + one, 256 + max(one, min(every, CAP)))
        at = 0
        for l0, l1 in blocks:
            assert l0 == at and l0 < l1
            at = l1
            assert integ(sum(sizes[l0:l1]), n_i) <= usable                                   # the integrals fit ...
            assert l1 == len(sizes) or integ(sum(sizes[l0:l1 + 1]), n_i) > usable             # ... and the next locus' would not
        assert at == len(sizes)


def test_posterior_loci_per_block_over_a_sweep(exe):
    rnd = random.Random(11)
    cases = []
    for _ in range(400):
        Wb, K, B, L = rnd.randrange(1, 40), rnd.choice([2, 3, 4, 8, 16]), rnd.choice([2, 3, 127, 128, 129, 300, 4096]), rnd.choice([0, 1, 5, 70000])
        cases += [(Wb, K, B, L, d) for d in (0, 1, 255, 256, 4096, 1 << 20, -1)]
    got = run_dump(exe, ["pp 4096 %d %d %d %d %d" % (d, Wb, K, B, L) for Wb, K, B, L, d in cases])
    for (Wb, K, B, L, d), (mn, pf, usable, nb) in zip(cases, got):
        fixed, one, every = 256 + au(8 * max(L, 1)), pp_block(1, K, B, Wb), pp_block(max(L, 1), K, B, Wb)
        assert mn == fixed + one and pf == fixed + max(one, min(every, CAP)) and mn <= pf <= fixed + max(one, CAP)
        assert usable == (pf if d < 0 else mn + d) - fixed + 256
        if L:
            assert 1 <= nb <= min(L, MAX_LOCI) and pp_block(nb, K, B, Wb) <= usable          # the block fits ...
            assert nb == min(L, MAX_LOCI) or pp_block(nb + 1, K, B, Wb) > usable             # ... and one more locus would not


def test_parboot_layout(exe):
    rnd = random.Random(3)
    cases = [(rnd.randrange(1, 70), rnd.choice([0, 1, 255, 256, 257, rnd.randrange(5000)]), rnd.randrange(0, 9), rnd.randrange(0, 40),
              rnd.choice([2, 3, 129, 4096]), rnd.choice([0, 1, 256, 123457])) for _ in range(300)]
    got = run_dump(exe, ["pb %d %d %d %d %d %d %d" % (nt, n, L, Wb + 7, Wb, B, ws) for nt, n, L, Wb, B, ws in cases])
    for (nt, n, L, Wb, B, ws), row in zip(cases, got):
        sizes = [nt * n, 8 * n, 8 * n, 8 * n, n, 4 * n, 8 * L * (Wb + 7), 8 * L * B * Wb, 8 * n, 8 * n, ws]
        at = 0
        for off, size in zip(row[:11], sizes):       # in order, aligned, none reaching into the next
            assert off == at and off % 256 == 0
            at = au(off + size)
        assert row[11] == at + 256                   # the total allows for aligning the caller's pointer up


def test_dump_program_under_sanitizers(tmp_path):
    """The block functions and the dump program once under AddressSanitizer and UBSan (a stand-alone executable)."""
    exe = build_dump(tmp_path, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    check_pinned(run_dump(exe, pinned_queries()))
    run_dump(exe, ["base 4097 10", "rs 4096 0 2 3 5 0 9", "pp 4096 0 6 4 130 3", "pp 4096 -1 6 4 130 0", "pb 4 10 2 9 6 5 1000"])


def test_the_drivers_ask_the_block_functions():
    """The three drivers keep no second copy of the alignment, the cap or the replicate limit, and the header stands alone."""
    for name in ("bootstrap_driver.hip", "simulate_driver.hip", "posterior_pi_driver.hip"):
        driver = open(os.path.join(CSRC, name)).read()
        for gone in ("1 << 30", "/ kBsAlign * kBsAlign", "kParbootMaxReplicates"):
            assert gone not in driver, (name, gone)
    header = open(os.path.join(CSRC, "band_blocks.hpp")).read()
    assert "#include <hip" not in header and '#include "' not in header      # g++ compiles it with nothing else of the project

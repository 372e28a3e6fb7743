"""The launch decisions of plan creation on the CPU: tapir_amd/csrc/site_launch_plan.hpp compiled with g++ into
tests/native/site_launch_dump.cpp, an occupancy table in place of the device query.  Every expected value below was worked
out by hand from the rules (their statement order included), for a device of 256 CUs; none comes from the code under test.
The workspace layout is restated here independently: region sizes in order, each rounded up to 256 bytes, plus 256.  So are the
arguments of every site-rate launch (site_kernel_args), which the launch code takes from the same header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSIMONY, REFERENCE = 2, 1           # TPHIP_START_* (include/tphip.h)
AUTO, OFF = 0, 1                      # TPHIP_DEDUP_* / DEDUP_*
STREAM, STREAM_SPILL, MIXED = -1, -2, 100   # launcher variants (launch_constants.hpp)
T, N_I = 50, 2


def lds(depth):        # one locus at a time: 160 doubles of tables, 12 x 64 doubles per parked partial
    return (160 + depth * 12 * 64) * 8


def mixed_lds(depth):  # mixed-loci mode: 8 x 64 + 64 + 32 doubles of tables
    return (8 * 64 + 64 + 32 + depth * 12 * 64) * 8


# shapes: ntaxa, nwords, stack depth, loci, columns per locus, occupancy table {(variant, LDS bytes): workgroups per CU}
SHAPES = {
    "A": (64, 8, 3, 100, 50000, {(8, 19712): 8}),
    "B": (64, 8, 3, 50000, 1000, {(8, 19712): 8}),
    "C": (256, 32, 4, 10000, 2000, {(STREAM, 25856): 6, (STREAM_SPILL, 19712): 8}),
    "D": (16, 2, 2, 1000, 500, {(2, 13568): 8, (MIXED + 2, 17152): 8}),
    "E": (64, 8, 3, 1900, 1000, {(8, 19712): 8, (MIXED + 8, 23296): 6}),
    "S": (64, 8, 3, 6, 2500, {(8, 19712): 8}),   # the batch of test_gpu_share_work.py
}
assert lds(3) == 19712 and lds(4) == 25856 and lds(2) == 13568 and mixed_lds(2) == 17152 and mixed_lds(3) == 23296

W = dict(w_slow=2970, w_easy=2089)    # round(2.9 * 1024), round(2.04 * 1024)
DEFAULTS = dict(chunk_cols=512, tail_order=1, mixed=0, mixed_few_waves=0, mixed_switch_cols=0, share_work=0, reserve_q=0,
                host_split=2, **W)


def case(shape, knobs, queries, **expected):
    return dict(shape=shape, knobs=knobs, queries=queries, expected=dict(DEFAULTS, **expected))


CASES = {
    # A: 5e6 columns / 2048 waves = 2441 per share (>= 1500: uneven, x3), inside loci of 50000 (< 2 loci: 0.8 up front, shares by
    # predicted work, reserve round(0.15 * 65536) = 9830); 98 slices and 49 PI chunks per locus; long loci: chunked compaction
    "A": case("A", {}, [(8, 19712)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=2048, persistent=1, grid_mult=3, lds_depth=3,
              first_fraction=0.8, share_work=1, reserve_q=9830, compact_chunked=1, n_site_chunks=9800, n_pi_chunks=4900, grid=6144),
    # B: 5e7 / 2048 = 24414 per share, 24 loci of 1000 each (>= 2 loci: 0.9 up front, equal column counts)
    "B": case("B", {}, [(8, 19712)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=2048, persistent=1, grid_mult=3, lds_depth=3,
              first_fraction=0.9, compact_chunked=0, n_site_chunks=100000, n_pi_chunks=50000, grid=6144),
    # C: 6 waves per CU with four parked partials in LDS, 8 with three: the spill variant, 2e7 / 2048 = 9765 per share; 0.8 up front
    # because of the spill; 2000 <= 2048: one workgroup per locus compacts; 2048 x 3 scratch rows of 6144 bytes
    "C": case("C", {}, [(STREAM, 25856), (STREAM_SPILL, 19712)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=2048, persistent=1,
              grid_mult=3, lds_depth=3, first_fraction=0.8, compact_chunked=0, n_site_chunks=40000, n_pi_chunks=20000, grid=6144),
    # D: 5e5 / 2048 = 244 per share: not persistent; mixed (16.8 estimated rounds, 8 waves per CU: two per SIMD, one below
    # int(24 * 65536 / 3.7) = 425098 work columns); HyPhy's start below 32 taxa; below 2^20 columns no de-duplication
    "D": case("D", {}, [(2, 13568), (MIXED + 2, 17152)], start_rule=REFERENCE, dedup_mode=OFF, waves=2048, persistent=0, mixed=1,
              mixed_few_waves=1024, mixed_switch_cols=425098, grid_mult=1, lds_depth=2, first_fraction=0.0, compact_chunked=0,
              n_site_chunks=1000, n_pi_chunks=1000, grid=2048),
    # E: 1.9e6 / 2048 = 927: not persistent; 1.9e6 * 1.4 / 65536 = 40.6 estimated rounds >= 28 with 6 < 8 waves per CU: slices
    "E": case("E", {}, [(8, 19712), (MIXED + 8, 23296)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=2048, persistent=0, grid_mult=1,
              lds_depth=3, first_fraction=0.0, compact_chunked=0, n_site_chunks=3800, n_pi_chunks=1900, grid=3800),
    # F: TPHIP_SITE_MIXED=1 forces the mode and switches the 28-rounds rule off: min(1024 SIMDs, 6 * 256) waves
    "F": case("E", {"TPHIP_SITE_MIXED": "1"}, [(8, 19712), (MIXED + 8, 23296)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=1024,
              persistent=0, mixed=1, mixed_few_waves=1024, mixed_switch_cols=655360, grid_mult=1, lds_depth=3, first_fraction=0.0,
              compact_chunked=0, n_site_chunks=3800, n_pi_chunks=1900, grid=1024),
    # G: no spill (and no query for it): 1536 waves, 13020 per share = 6 loci: 0.9 up front
    "G": case("C", {"TPHIP_SITE_SPILL": "0"}, [(STREAM, 25856)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=1536, persistent=1,
              grid_mult=3, lds_depth=4, first_fraction=0.9, compact_chunked=0, n_site_chunks=40000, n_pi_chunks=20000, grid=4608),
    # H: BASE + WORK of test_gpu_share_work.py on its 6 x 2500 batch: 15000 / 2048 = 7 per share, persistent by the knob only;
    # 16 waves: 937 per share (< 1500: the multiplier, the fraction and shares by work come from the knobs alone); reserve 0.25
    "H": case("S", {"TPHIP_SITE_PERSISTENT": "1", "TPHIP_SITE_WAVES": "16", "TPHIP_SITE_GRID_MULT": "3", "TPHIP_SITE_FIRST_FRACTION": "0.8",
                    "TPHIP_SITE_SHARE_WORK": "1", "TPHIP_SITE_RESERVE": "0.25", "TPHIP_SITE_CLASS_WEIGHTS": "2.9,2.04"},
              [(8, 19712)], start_rule=PARSIMONY, dedup_mode=OFF, waves=16, persistent=1, grid_mult=3, lds_depth=3, first_fraction=0.8,
              share_work=1, reserve_q=16384, compact_chunked=1, n_site_chunks=30, n_pi_chunks=18, grid=48),
    # I: A without shares by predicted work: no reserve, so no second work list either
    "I": case("A", {"TPHIP_SITE_SHARE_WORK": "0"}, [(8, 19712)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=2048, persistent=1,
              grid_mult=3, lds_depth=3, first_fraction=0.8, compact_chunked=1, n_site_chunks=9800, n_pi_chunks=4900, grid=6144),
    # J: B with the chunk-parallel compaction forced onto its short loci
    "J": case("B", {"TPHIP_COMPACT_CHUNKED": "1"}, [(8, 19712)], start_rule=PARSIMONY, dedup_mode=AUTO, waves=2048, persistent=1,
              grid_mult=3, lds_depth=3, first_fraction=0.9, compact_chunked=1, n_site_chunks=100000, n_pi_chunks=50000, grid=6144),
    # K: TPHIP_SITE_WAVES comes after the mixed decision: the mode stays, the grid is the knob's, the switch to few waves is off
    "K": case("D", {"TPHIP_SITE_WAVES": "100"}, [(2, 13568), (MIXED + 2, 17152)], start_rule=REFERENCE, dedup_mode=OFF, waves=100,
              persistent=0, mixed=1, mixed_few_waves=1024, mixed_switch_cols=0, grid_mult=1, lds_depth=2, first_fraction=0.0,
              compact_chunked=0, n_site_chunks=1000, n_pi_chunks=1000, grid=100),
    # L: TPHIP_SITE_PERSISTENT=0 comes after the spill variant was chosen (and asked for) and takes it back: slices of C
    "L": case("C", {"TPHIP_SITE_PERSISTENT": "0"}, [(STREAM, 25856), (STREAM_SPILL, 19712)], start_rule=PARSIMONY, dedup_mode=AUTO,
              waves=1536, persistent=0, grid_mult=1, lds_depth=4, first_fraction=0.0, compact_chunked=0, n_site_chunks=40000,
              n_pi_chunks=20000, grid=40000),
    # M: values outside the accepted ranges leave A as it is (slice length < 64, multiplier > 16, a class weight > 16); a reserve above
    # 1 is cut to 1; switches
    "M": case("A", {"TPHIP_SITE_CHUNK": "32", "TPHIP_SITE_GRID_MULT": "17", "TPHIP_SITE_CLASS_WEIGHTS": "17,1", "TPHIP_SITE_RESERVE": "1.5",
                    "TPHIP_SITE_TAIL_ORDER": "0", "TPHIP_DEDUP": "0", "TPHIP_HOST_SPLIT": "100"},
              [(8, 19712)], start_rule=PARSIMONY, dedup_mode=OFF, waves=2048, persistent=1, grid_mult=3, lds_depth=3, first_fraction=0.8,
              tail_order=0, share_work=1, reserve_q=65536, compact_chunked=1, host_split=64, n_site_chunks=9800, n_pi_chunks=4900, grid=6144),
}


# What launch_site_rates hands to the kernel at every launch (site_kernel_args), worked out by hand from the decisions above and
# the rules, in their order:
#   variant      2 / 8 words in registers, else the streamed words (STREAM; STREAM_SPILL when lds_depth < stack depth); MIXED + in mixed mode
#   LDS          lds(lds_depth), mixed_lds(stack depth) in mixed mode
#   grid         waves in mixed mode, the slices (n_site_chunks) when not persistent, else waves x grid_mult (no case has later shares
#                spelled out by the knob, which alone make it larger)
#   persistent   persistent or mixed;  first_round = waves;  tail_order only when persistent, not mixed and not switched off
#   fraction     first_fraction where > 0, else 1 / grid_mult; then 1.0 in mixed mode
#   main_shares  waves with reserved tails (reserve_q > 0), else waves x grid_mult
#   second_list  whenever the plan is not persistent (the mixed mode is not: it only launches as persistent)
# columns: variant, LDS bytes, grid, persistent, first_round, first_fraction, tail_order, share_work, main_shares, spill, second_list
ARG_KEYS = ("variant", "lds_bytes", "grid", "persistent", "first_round", "first_fraction", "tail_order", "share_work", "main_shares",
            "spill", "second_list")
LAUNCH_ARGS = {
    "A": (8, lds(3), 6144, 1, 2048, 0.8, 1, 1, 2048, 0, 0),        # reserve 9830 > 0: the 2048 first shares are the main ones
    "B": (8, lds(3), 6144, 1, 2048, 0.9, 1, 0, 6144, 0, 0),        # no reserve: all 2048 x 3 shares are main shares
    "C": (STREAM_SPILL, lds(3), 6144, 1, 2048, 0.8, 1, 0, 6144, 1, 0),   # 32 words, three of four partials in LDS
    "D": (MIXED + 2, mixed_lds(2), 2048, 1, 2048, 1.0, 0, 0, 2048, 0, 1),   # 0.0 -> 1 / 1, and 1.0 anyway; not persistent: second list
    "E": (8, lds(3), 3800, 0, 2048, 1.0, 0, 0, 2048, 0, 1),        # slices: the grid is the 3800 slices; 0.0 -> 1 / 1
    "F": (MIXED + 8, mixed_lds(3), 1024, 1, 1024, 1.0, 0, 0, 1024, 0, 1),
    "G": (STREAM, lds(4), 4608, 1, 1536, 0.9, 1, 0, 4608, 0, 0),   # lds_depth = stack depth: no spill
    "H": (8, lds(3), 48, 1, 16, 0.8, 1, 1, 16, 0, 0),              # reserve 16384 > 0: 16 main shares of 48
    "I": (8, lds(3), 6144, 1, 2048, 0.8, 1, 0, 6144, 0, 0),        # A without the reserve
    "J": (8, lds(3), 6144, 1, 2048, 0.9, 1, 0, 6144, 0, 0),        # as B: the compaction is not the kernel's business
    "K": (MIXED + 2, mixed_lds(2), 100, 1, 100, 1.0, 0, 0, 100, 0, 1),
    "L": (STREAM, lds(4), 40000, 0, 1536, 1.0, 0, 0, 1536, 0, 1),  # the spill taken back: 40000 slices, 1536 x 1 main shares
    "M": (8, lds(3), 6144, 1, 2048, 0.8, 0, 1, 2048, 0, 0),        # A with TPHIP_SITE_TAIL_ORDER=0
}
assert sorted(LAUNCH_ARGS) == sorted(CASES)
BASE_VARIANT = {2: 2, 8: 8, 32: STREAM}   # site_variant by the shape's packed words


def build_dump(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "site_launch_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + os.path.join(ROOT, "tapir_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "site_launch_dump.cpp"), "-o", exe])
    return exe


def dump_input(c):
    ntaxa, nwords, depth, nloci, cols, occ = SHAPES[c["shape"]]
    lines = ["shape %d %d %d 0 0 0 0 %d %d" % (ntaxa, nwords, depth, T, N_I), "cus 256", "loci %d %d" % (nloci, cols)]
    lines += ["knob %s %s" % kv for kv in c["knobs"].items()]
    lines += ["occ %d %d %d" % (v, b, n) for (v, b), n in occ.items()]
    return "\n".join(lines) + "\n"


def run_dump(exe, c):
    text = subprocess.run([exe], input=dump_input(c), capture_output=True, text=True, check=True).stdout
    return dict(line.split(" ", 1) for line in text.splitlines())


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    exe = build_dump(tmp_path_factory.mktemp("site_launch"))
    return {name: run_dump(exe, c) for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_decisions(dumped, name):
    got, c = dumped[name], CASES[name]
    for key, want in c["expected"].items():
        assert float(got[key]) == want, (name, key, got[key], want)
    assert got["queries"].split() == ["%d:%d" % q for q in c["queries"]], name
    assert got["chunk_tables_ok"] == "1"
    assert int(got["lds_bytes"]) == lds(c["expected"]["lds_depth"])
    assert int(got["mixed_lds_bytes"]) == mixed_lds(SHAPES[c["shape"]][2])


def check_launch_args(got, name):
    for key, want in zip(ARG_KEYS, LAUNCH_ARGS[name]):
        assert float(got["args." + key]) == want, (name, key, got["args." + key], want)
    assert int(got["site_variant"]) == BASE_VARIANT[SHAPES[CASES[name]["shape"]][1]]
    assert int(got["args.grid"]) == CASES[name]["expected"]["grid"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_arguments(dumped, name):
    check_launch_args(dumped[name], name)


def test_dump_program_under_sanitizers(tmp_path):
    """Every case once more through the decision code and the launch arguments under AddressSanitizer and UBSan (a stand-alone
    executable)."""
    exe = build_dump(tmp_path, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name in sorted(CASES):
        got, c = run_dump(exe, CASES[name]), CASES[name]
        for key, want in c["expected"].items():
            assert float(got[key]) == want, (name, key, got[key], want)
        check_launch_args(got, name)


def restated_layout(c):
    """The regions of the workspace, in order, from the case's shape and its expected decisions."""
    ntaxa, nwords, depth, nloci, cols, _ = SHAPES[c["shape"]]
    e, n, npc = c["expected"], nloci * cols, c["expected"]["n_pi_chunks"]
    regions = [("work_cols", 4 * n)]
    if not e["persistent"] or e["reserve_q"] > 0:
        regions.append(("work_cols2", 4 * n))
    regions += [("work_count", 4 * nloci), ("work_prefix", 8 * (nloci + 1)), ("slice_prefix", 8 * (nloci + 1)), ("work_class", 8 * nloci),
                ("work_wprefix", 8 * (nloci + 1)), ("part_prefix", 16 * (nloci + 1)), ("part_start", 16 * (nloci + 1)),
                ("chunk_cnt", 8 * max(1, npc)), ("partial", 8 * npc * (T + 2 * N_I)), ("packed", 4 * nwords * n)]
    if e["dedup_mode"] != OFF:
        regions += [("hash", 8 * n), ("dup_of", 4 * n), ("tab_key", 16 * n), ("tab_val", 8 * n), ("dedup_on", 4 * nloci)]
    if e["lds_depth"] < depth:
        regions.append(("spill", e["waves"] * e["grid_mult"] * (depth - e["lds_depth"]) * 12 * 64 * 8))
    return regions


ALL_REGIONS = ("work_cols", "work_cols2", "work_count", "work_prefix", "slice_prefix", "work_class", "work_wprefix", "part_prefix",
               "part_start", "chunk_cnt", "partial", "packed", "hash", "dup_of", "tab_key", "tab_val", "dedup_on", "spill")


@pytest.mark.parametrize("name", sorted(CASES))
def test_workspace_layout(dumped, name):
    got, c = dumped[name], CASES[name]
    regions, off, spans = restated_layout(c), 0, []
    for region, size in regions:
        assert int(got["ws." + region]) == off, (name, region)
        spans.append((off, off + size))
        off = (off + size + 255) // 256 * 256
    assert int(got["ws.total"]) == off + 256
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):     # in order, 256-aligned, no overlap
        assert a0 % 256 == 0 and a1 <= b0
    assert spans[-1][1] <= int(got["ws.total"])
    present = {region for region, _ in regions}
    for region in ALL_REGIONS:                           # the launch code tests work_cols2 for zero
        if region not in present:
            assert int(got["ws." + region]) == 0, (name, region)


def test_presence_of_optional_regions_as_listed():
    """What the case list says about the optional regions, against the restated layout (which follows the expected decisions)."""
    has = {n: {r for r, _ in restated_layout(CASES[n])} for n in CASES}
    assert "work_cols2" in has["A"] and "work_cols2" not in has["B"] and "work_cols2" in has["D"] and "work_cols2" in has["E"]
    assert "hash" in has["A"] and "hash" not in has["D"]
    assert "spill" not in has["A"] and "spill" not in has["G"] and "work_cols2" not in has["I"]
    assert dict(restated_layout(CASES["C"]))["spill"] == 6144 * 6144 == 37748736


def test_decision_code_reads_no_environment():
    """The knobs reach the decisions through PlanKnobs only: no getenv in the header, none in tphip_plan_create, and the LDS
    formulas are written once."""
    csrc = os.path.join(ROOT, "tapir_amd", "csrc")
    header = open(os.path.join(csrc, "site_launch_plan.hpp")).read()
    assert "getenv" not in header and "hip/" not in header
    tphip = open(os.path.join(csrc, "tphip.hip")).read()
    body = tphip[tphip.index("int tphip_plan_create("):tphip.index("int32_t tphip_plan_table_width")]
    assert "getenv" not in body
    for name in os.listdir(csrc):
        if name.endswith(".hip"):
            assert "12 * kSiteBlock) * sizeof(double)" not in open(os.path.join(csrc, name)).read(), name


def test_variant_rule_is_written_once():
    """The launcher variant by the packed words is site_variant in the decision header; no .hip file restates it."""
    csrc = os.path.join(ROOT, "tapir_amd", "csrc")
    assert open(os.path.join(csrc, "site_launch_plan.hpp")).read().count("nwords <= 2 ? 2") == 1
    hips = [name for name in os.listdir(csrc) if name.endswith(".hip")]
    assert "site_driver.hip" in hips and "eb_driver.hip" in hips
    for name in hips:
        assert "nwords <= 2 ? 2" not in open(os.path.join(csrc, name)).read(), name
    assert "site_variant(" in open(os.path.join(csrc, "eb_driver.hip")).read()
    assert "site_kernel_args(" in open(os.path.join(csrc, "site_driver.hip")).read()

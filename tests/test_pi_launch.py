"""How a plan runs its PI partial sums, decided on the CPU: SiteLaunch::pi_split of tapir_amd/csrc/site_launch_plan.hpp compiled
with g++ into tests/native/pi_launch_dump.cpp.  Long loci (max_locus_cols > 2048, the chunked compaction's rule) take
pi_net_kernel + pi_interval_kernel, everything else the fused pi_partial_kernel; TPHIP_PI_SPLIT=0/1 overrides both ways.  The two
paths write the same `partial` region and nothing else, so the workspace layout does not depend on the choice; the region's
size is restated here (8 bytes x PI chunks x (T + 2 n_i), rounded up to 256)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tapir_amd", "csrc")
T, N_I = 50, 4

# name: (ntaxa, packed words, stack depth, [(loci, columns each), ...], knobs, expected pi_split)
CASES = {
    "at_2048": (64, 8, 3, [(3, 2048)], {}, 0),
    "at_2049": (64, 8, 3, [(3, 2048), (1, 2049)], {}, 1),
    "one_long_among_short": (16, 2, 2, [(40, 500), (1, 5000), (40, 500)], {}, 1),
    "C2": (16, 2, 2, [(1000, 500)], {}, 0),
    "C3": (64, 8, 3, [(100, 50000)], {}, 1),
    "C4": (64, 8, 3, [(50000, 1000)], {}, 0),
    "C5": (256, 32, 4, [(10000, 2000)], {}, 0),
    "C3_knob_off": (64, 8, 3, [(100, 50000)], {"TPHIP_PI_SPLIT": "0"}, 0),
    "C2_knob_on": (16, 2, 2, [(1000, 500)], {"TPHIP_PI_SPLIT": "1"}, 1),
    "at_2048_knob_on": (64, 8, 3, [(3, 2048)], {"TPHIP_PI_SPLIT": "1"}, 1),
    "at_2049_knob_off": (64, 8, 3, [(3, 2048), (1, 2049)], {"TPHIP_PI_SPLIT": "0"}, 0),
    # the knob is its own: the compaction's switch does not move it, and it does not move the compaction's
    "C2_compaction_knob": (16, 2, 2, [(1000, 500)], {"TPHIP_COMPACT_CHUNKED": "1"}, 0),
}
COMPACT_CHUNKED = {"C2_compaction_knob": 1, "C3_knob_off": 1, "C2_knob_on": 0, "at_2048_knob_on": 0, "at_2049_knob_off": 1}


def build_dump(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "pi_launch_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "pi_launch_dump.cpp"), "-o", exe])
    return exe


def dump_input(case):
    ntaxa, nwords, depth, loci, knobs, _ = case
    lines = ["shape %d %d %d %d %d" % (ntaxa, nwords, depth, T, N_I), "cus 256"]
    lines += ["loci %d %d" % lc for lc in loci]
    lines += ["knob %s %s" % kv for kv in knobs.items()]
    return "\n".join(lines) + "\n"


def run_dump(exe, case):
    text = subprocess.run([exe], input=dump_input(case), capture_output=True, text=True, check=True).stdout
    return dict(line.split(" ", 1) for line in text.splitlines())


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    exe = build_dump(tmp_path_factory.mktemp("pi_launch"))
    return {name: run_dump(exe, case) for name, case in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pi_split_decision(dumped, name):
    got, case = dumped[name], CASES[name]
    assert int(got["max_locus_cols"]) == max(c for _, c in case[3])
    assert int(got["pi_split"]) == case[5], name
    want_compact = COMPACT_CHUNKED.get(name, 1 if int(got["max_locus_cols"]) > 2048 else 0)
    assert int(got["compact_chunked"]) == want_compact, name


def n_pi_chunks(case):
    return sum(n * ((c + 1023) // 1024) for n, c in case[3])


@pytest.mark.parametrize("pair", [("C3", "C3_knob_off"), ("C2", "C2_knob_on"), ("at_2048", "at_2048_knob_on"),
                                  ("at_2049", "at_2049_knob_off")], ids=lambda p: p[0])
def test_workspace_layout_does_not_depend_on_the_split(dumped, pair):
    """No buffer is handed from pi_net_kernel to pi_interval_kernel: every region sits where it sat, and `partial` has its size."""
    a, b = dumped[pair[0]], dumped[pair[1]]
    assert int(a["pi_split"]) != int(b["pi_split"])
    regions = sorted(k for k in a if k.startswith("ws."))
    assert len(regions) == 19 and regions == sorted(k for k in b if k.startswith("ws."))
    for k in regions:
        assert a[k] == b[k], (pair, k)
    npc = n_pi_chunks(CASES[pair[0]])
    assert int(a["n_pi_chunks"]) == npc
    size = 8 * npc * (T + 2 * N_I)
    assert int(a["ws.packed"]) - int(a["ws.partial"]) == (size + 255) // 256 * 256
    assert int(a["ws.partial"]) % 256 == 0 and int(a["ws.partial"]) > int(a["ws.chunk_cnt"])


def test_dump_program_under_sanitizers(tmp_path):
    """The decision code and the dump program once under AddressSanitizer and UBSan (a stand-alone executable), on the case
    with the most loci and on a knob case."""
    exe = build_dump(tmp_path, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name in ("C4", "C2_knob_on"):
        got = run_dump(exe, CASES[name])
        assert int(got["pi_split"]) == CASES[name][5]


def test_knob_goes_through_plan_knobs_only():
    """TPHIP_PI_SPLIT is read where every plan knob is read (the list of names walked by knobs_from_env): no getenv in the
    decision header or in the kernels' header, and the launch code asks the plan, not the environment."""
    header = open(os.path.join(CSRC, "site_launch_plan.hpp")).read()
    assert '"TPHIP_PI_SPLIT"' in header[header.index("kPlanKnobNames"):header.index("set_plan_knob")]
    assert "getenv" not in header
    assert "getenv" not in open(os.path.join(CSRC, "pi_kernels.hpp")).read()
    units = {name: open(os.path.join(CSRC, name)).read() for name in os.listdir(CSRC) if name.endswith(".hip")}
    assert all("TPHIP_PI_SPLIT" not in text for text in units.values())
    driver = units["site_driver.hip"]
    body = driver[driver.index("int launch_pi_tables("):driver.index("static int take_slot(")]
    assert "p->site.pi_split" in body and "getenv" not in body
    for kernel in ("pi_net_kernel<<<", "pi_interval_kernel<<<", "pi_partial_kernel<<<"):
        assert sum(text.count(kernel) for text in units.values()) == 1 and kernel in body, kernel

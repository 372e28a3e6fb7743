"""How the column simulation is launched, decided on the CPU: sim_launch_shape of tapir_amd/csrc/simulate_launch_shape.hpp
compiled with g++ into tests/native/sim_launch_dump.cpp.  The kernel keeps ceil(nint / 16) packed words per column in LDS, so the
block shrinks from 256 to 128 to 64 threads as the internal nodes grow, a launch above 48 KiB has to raise the kernel's limit
first, and a tree with more than 10240 internal nodes is refused.  The expected values are restated here from that rule, not read
from the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tapir_amd", "csrc")

# nint: (accepted, block, LDS bytes, above the 48 KiB line)
EDGES = {
    1: (1, 256, 1024, 0),
    16: (1, 256, 1024, 0),
    17: (1, 256, 2048, 0),
    768: (1, 256, 49152, 0),
    769: (1, 256, 50176, 1),      # 49 words x 256 threads x 4 bytes (51200 would be 50 words: 785 to 800 nodes)
    800: (1, 256, 51200, 1),
    2560: (1, 256, 163840, 1),
    2561: (1, 128, 82432, 1),
    5120: (1, 128, 163840, 1),
    5121: (1, 64, 82176, 1),
    10240: (1, 64, 163840, 1),
    10241: (0, 64, 164096, 1),
    131071: (0, 64, 2097152, 1),
}
LDS_LIMIT = 160 * 1024


def build_dump(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "sim_launch_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "sim_launch_dump.cpp"), "-o", exe])
    return exe


def run_dump(exe, counts):
    text = subprocess.run([exe], input="".join("%d\n" % n for n in counts), capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(v) for v in line.split()) for line in text.splitlines()]
    assert [r[0] for r in rows] == list(counts)
    return {r[0]: r[1:] for r in rows}


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    exe = build_dump(tmp_path_factory.mktemp("sim_launch"))
    return run_dump(exe, list(range(0, 10300)) + [131071])


@pytest.mark.parametrize("nint", sorted(EDGES))
def test_launch_shape_at_its_edges(dumped, nint):
    ok, words, block, lds, raised = dumped[nint]
    print("nint %d: ok %d, words %d, block %d, LDS %d, raised %d" % (nint, ok, words, block, lds, raised))
    assert (ok, block, lds, raised) == EDGES[nint]
    assert words == (nint + 15) // 16


def test_every_accepted_shape_fits_the_lds(dumped):
    """Every count from 0 to 10299: the words hold every slot, the block is the largest of 256, 128, 64 that fits, LDS never
    exceeds 160 KiB on an accepted shape, and the refusal starts at 10241 and never ends."""
    for nint in range(0, 10300):
        ok, words, block, lds, raised = dumped[nint]
        assert words * 16 >= nint > (words - 1) * 16 or nint == 0 and words == 0
        assert block in (64, 128, 256) and lds == 4 * words * block and raised == (lds > 48 * 1024)
        assert ok == (nint <= 10240)
        if ok:
            assert lds <= LDS_LIMIT
            assert block == 256 or 4 * words * 2 * block > LDS_LIMIT      # a larger block would not fit


def test_dump_program_under_sanitizers(tmp_path):
    """The shape function and the dump program once under AddressSanitizer and UBSan (a stand-alone executable)."""
    exe = build_dump(tmp_path, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    got = run_dump(exe, sorted(EDGES))
    for nint, want in EDGES.items():
        assert (got[nint][0],) + got[nint][2:] == want


def test_the_driver_asks_the_shape_function():
    """sim_prepare and sim_launch take words, block, the refusal and the 48 KiB line from the header: no second copy of the rule."""
    driver = open(os.path.join(CSRC, "simulate_driver.hip")).read()
    prepare = driver[driver.index("int sim_prepare("):driver.index("int sim_stage_ids(")]
    launch = driver[driver.index("int sim_launch("):driver.index("struct ParbootLayout")]
    assert "sim_launch_shape(nint, &words, &block)" in prepare and "kSimLdsBytes" not in prepare and ">>=" not in prepare
    assert "sim_lds_bytes(p->sim_words, p->sim_block)" in launch and "kSimLdsDefaultBytes" in launch and "48 * 1024" not in launch
    header = open(os.path.join(CSRC, "simulate_launch_shape.hpp")).read()
    assert "#include <hip" not in header and '#include "' not in header      # g++ compiles it with nothing else of the project

"""The stage-1 launch decisions of plan creation and the arithmetic of a call, on the CPU: tapir_amd/csrc/locus_launch_plan.hpp
compiled with g++ into tests/native/locus_launch_dump.cpp, tables in place of the kernels' LDS and occupancy queries.  The expected
values of the named cases were worked out by hand from the rules; every case is also held against `restated` below, the same
rules written out independently (sizes in bytes, blocks of 128 threads, 256 CUs).  Unless a case says otherwise every LDS request
is allowed and every occupancy query answers 4."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tapir_amd", "csrc")
KIB = 1024
CUS = 256


def shape(ntaxa=16, nnodes=None, nwords=None, depth=3, ntape=14, cols=600, value_nops=20, built=1, rdepth=4, ntape2=None):
    nnodes = 2 * ntaxa - 1 if nnodes is None else nnodes
    return dict(ntaxa=ntaxa, nnodes=nnodes, nwords=(ntaxa + 7) // 8 if nwords is None else nwords, depth=depth, ntape=ntape, cols=cols,
                value_nops=value_nops, built=built, rdepth=rdepth, ntape2=ntaxa - 2 if ntape2 is None else ntape2)


def restated(sh, knobs=None, deny=(), occ=4):
    """The decisions, their queries in order, from the rules.  deny: kernels whose LDS request fails; occ: {kernel: answer} or one
    answer for both gradient kernels (0 = the query fails)."""
    knobs, q, e = knobs or {}, [], {}
    occ_of = (lambda k: occ.get(k, 4)) if isinstance(occ, dict) else (lambda k: occ)
    nn, nt, nw, d = sh["nnodes"], sh["ntaxa"], sh["nwords"], sh["depth"]

    def allow(kernel, limit, *args):
        q.append(" ".join(["allow", kernel] + [str(a) for a in args] + [str(limit)]))
        return kernel not in deny

    # eigenbasis value kernel: e^{lambda t} per node, the stack of parked partials
    e["lik_lds"] = 8 * (4 * nn + 4 * 128 * d)
    e["lik_ok"] = int(e["lik_lds"] <= 150 * KIB and (e["lik_lds"] <= 64 * KIB or allow("lik", 150 * KIB)))
    # transition-matrix value kernel: 20 doubles per taxon, one packed word per 8 tips, column and thread
    cols = 2 if sh["cols"] >= 512 else 1
    if "TPHIP_VALUE_COLS" in knobs:
        cols = 2 if int(knobs["TPHIP_VALUE_COLS"]) >= 2 else 1
    e["value_cols"] = e["value_lds"] = 0
    if sh["value_nops"] > 0 and d <= 5 and "TPHIP_VALUE_EIGENBASIS" not in knobs:
        need = 160 * nt + 4 * 128 * nw * cols
        if need <= 96 * KIB and (need <= 64 * KIB or allow("value", 96 * KIB, cols, d)):
            e["value_cols"], e["value_lds"] = cols, need
    # eigenbasis gradient kernel: 12 doubles of tables per node and two accumulators per wave and address
    slots = 4
    while slots > 1 and 8 * nn * (12 + 4 * slots) > 100 * KIB:
        slots //= 2
    lds = 8 * nn * (12 + 4 * slots)
    stage = int(128 * nt <= 48 * KIB and lds + 128 * nt <= 150 * KIB)
    lds += 128 * nt * stage
    ok = lds <= 150 * KIB and (lds <= 64 * KIB or allow("grad", 150 * KIB))
    bpc = 1
    if ok:
        q.append("occ grad %d" % lds)
        bpc = max(1, occ_of("grad"))
        if max(1, sh["ntape"] + d) * 4 * 128 * 8 * CUS * bpc > 300 << 20:
            bpc = min(bpc, 3)
    e.update(grad_slots=slots, grad_stage=stage, grad_lds=lds, grad_ok=int(ok), grad_blocks_per_cu=bpc)
    # transition-matrix gradient kernel
    e.update(grad2_ok=0, grad2_lds=0, grad2_blocks_per_cu=1)
    if sh["built"]:
        lds2 = 8 * (20 * nt + 64 + 4 * 128 * sh["rdepth"] + 4 * nn) + 4 * 128 * nw
        e["grad2_lds"] = lds2
        if e["value_cols"] > 0 and lds2 <= 96 * KIB and (lds2 <= 64 * KIB or allow("grad2", 96 * KIB, d)):
            e["grad2_ok"] = 1
            q.append("occ grad2 %d %d" % (d, lds2))
            e["grad2_blocks_per_cu"] = max(1, occ_of("grad2"))
    return e, q


A = shape()
C511, C512 = shape(ntaxa=400, nwords=50, cols=511, depth=5), shape(ntaxa=400, nwords=50, cols=512, depth=5)
BIG2 = shape(ntaxa=200, nnodes=399, nwords=25, rdepth=8)   # grad2 between 64 and 96 KiB
# name: (shape, knobs, kernels denied, occupancy, expected fields, expected queries or None = the restatement's)
CASES = {
    "A": (A, {}, (), 4, dict(lik_lds=13280, lik_ok=1, value_cols=2, value_lds=4608, grad_slots=4, grad_stage=1, grad_lds=8992, grad_ok=1,
                             grad2_lds=21472, grad2_ok=1, grad_blocks_per_cu=4, grad2_blocks_per_cu=4), ["occ grad 8992", "occ grad2 3 21472"]),
    "B_511": (shape(cols=511), {}, (), 4, dict(value_cols=1), None),
    "B_512": (shape(cols=512), {}, (), 4, dict(value_cols=2), None),
    "B_512_knob_1": (shape(cols=512), {"TPHIP_VALUE_COLS": "1"}, (), 4, dict(value_cols=1, value_lds=2560 + 1024), None),
    "B_511_knob_3": (shape(cols=511), {"TPHIP_VALUE_COLS": "3"}, (), 4, dict(value_cols=2), None),
    "B_eigenbasis_0": (A, {"TPHIP_VALUE_EIGENBASIS": "0"}, (), 4, dict(value_cols=0, value_lds=0, grad2_ok=0, grad2_lds=21472), ["occ grad 8992"]),
    "B_no_value_program": (shape(value_nops=0), {}, (), 4, dict(value_cols=0, grad2_ok=0), ["occ grad 8992"]),
    "B_depth_6": (shape(depth=6), {}, (), 4, dict(value_cols=0, grad2_ok=0), None),
    "C_511": (C511, {}, (), 4, dict(value_cols=1, value_lds=89600), None),
    "C_511_denied": (C511, {}, ("value",), 4, dict(value_cols=0, value_lds=0, grad2_ok=0), None),
    "C_512": (C512, {}, (), 4, dict(value_cols=0, value_lds=0), None),   # 115200 bytes: no query, no fall-back to one column
    "D_457": (shape(ntaxa=229, nnodes=457), {}, (), 4, dict(grad_slots=4), None),
    "D_459": (shape(ntaxa=230, nnodes=459), {}, (), 4, dict(grad_slots=2, grad_stage=1, grad_lds=102880, grad_ok=1), None),
    "D_459_denied": (shape(ntaxa=230, nnodes=459), {}, ("grad",), 4, dict(grad_slots=2, grad_lds=102880, grad_ok=0, grad_blocks_per_cu=1), None),
    "D_641": (shape(ntaxa=321, nnodes=641), {}, (), 4, dict(grad_slots=1, grad_stage=1, grad_lds=82048 + 41088), None),
    "E_384": (shape(ntaxa=384, nnodes=767), {}, (), 4, dict(grad_slots=1, grad_stage=1, grad_lds=98176 + 49152, grad_ok=1), None),
    "E_385": (shape(ntaxa=385, nnodes=769), {}, (), 4, dict(grad_stage=0, grad_lds=769 * 16 * 8), None),
    "F": (shape(ntaxa=601, nnodes=1201), {}, (), 4, dict(grad_ok=0, grad_stage=0, grad_blocks_per_cu=1), None),
    "G_75": (shape(ntape=72, depth=3), {}, (), 4, dict(grad_blocks_per_cu=4), None),
    "G_76": (shape(ntape=73, depth=3), {}, (), 4, dict(grad_blocks_per_cu=3), None),
    "G_76_occ_2": (shape(ntape=73, depth=3), {}, (), 2, dict(grad_blocks_per_cu=2, grad2_blocks_per_cu=2), None),
    "G_occ_fails": (shape(ntape=73, depth=3), {}, (), 0, dict(grad_blocks_per_cu=1, grad2_blocks_per_cu=1), None),
    "H_not_built": (shape(built=0), {}, (), 4, dict(grad2_ok=0, grad2_lds=0, value_cols=2), ["occ grad 8992"]),
    "H_too_large": (shape(ntaxa=400, nwords=50, cols=511, depth=5, rdepth=8), {}, (), 4, dict(value_cols=1, grad2_ok=0), None),
    "H_between": (BIG2, {}, (), 4, dict(grad2_ok=1), None),
    "H_between_denied": (BIG2, {}, ("grad2",), 4, dict(grad2_ok=0, grad2_blocks_per_cu=1), None),
    "lik_above_64k": (shape(ntaxa=1500, nnodes=2999, nwords=188, depth=5, value_nops=0, built=0), {}, (), 4, dict(lik_ok=1, lik_lds=8 * (4 * 2999 + 2560)), None),
    "lik_denied": (shape(ntaxa=1500, nnodes=2999, nwords=188, depth=5, value_nops=0, built=0), {}, ("lik",), 4, dict(lik_ok=0), None),
    "lik_too_large": (shape(ntaxa=2400, nnodes=4799, nwords=300, depth=5, value_nops=0, built=0), {}, (), 4, dict(lik_ok=0), None),
}
NSPLIT = [(8, 300, 256, 2), (1616, 20000, 128, 2), (4096, 20000, 128, 1), (1, 10 ** 7, 128, 2048), (1, 50, 128, 1)]
# (items, nnodes, dlogt, d2logt): offsets of lnl, sum_dlogt, dexch, dlogt, d2logt and the total, in doubles
LAYOUT = [((6, 15, 0, 0), (0, 6, 12, 48, 48, 48)), ((6, 15, 1, 0), (0, 6, 12, 48, 138, 138)), ((6, 15, 0, 1), (0, 6, 12, 48, 48, 138)),
          ((6, 15, 1, 1), (0, 6, 12, 48, 138, 228))]


def build_dump(out_dir, extra=()):
    exe = os.path.join(str(out_dir), "locus_launch_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "locus_launch_dump.cpp"), "-o", exe])
    return exe


def dump_input(case):
    sh, knobs, deny, occ = case[:4]
    want, _ = restated(sh, knobs, deny, occ)
    lines = ["shape %d %d %d %d %d %d %d %d %d %d" % (sh["ntaxa"], sh["nnodes"], sh["nwords"], sh["depth"], sh["ntape"], sh["cols"],
                                                    sh["value_nops"], sh["built"], sh["rdepth"], sh["ntape2"]), "cus %d" % CUS]
    lines += ["knob %s %s" % kv for kv in knobs.items()]
    lines += ["allow %s %d %d" % (k, lim * KIB, k not in deny) for k, lim in (("lik", 150), ("value", 96), ("grad", 150), ("grad2", 96))]
    occ_of = (lambda k: occ.get(k, 4)) if isinstance(occ, dict) else (lambda k: occ)
    lines += ["occ %s %d %d" % (k, want[k + "_lds"], occ_of(k)) for k in ("grad", "grad2") if occ_of(k)]   # (0: the query fails)
    lines += ["nsplit %d %d %d" % t[:3] for t in NSPLIT] + ["layout %d %d %d %d" % t for t, _ in LAYOUT]
    return "\n".join(lines) + "\n"


def run_dump(exe, case):
    text = subprocess.run([exe], input=dump_input(case), capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(line.split(" ", 1) if " " in line else (line, "") for line in text if " -> " not in line)
    got["answers"] = [line for line in text if " -> " in line]
    return got


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    exe = build_dump(tmp_path_factory.mktemp("locus_launch"))
    return {name: run_dump(exe, case) for name, case in CASES.items()}


def check_case(got, name):
    sh, knobs, deny, occ, expected, queries = CASES[name]
    want, q = restated(sh, knobs, deny, occ)
    for key, value in expected.items():      # the hand-derived figures, against the restatement as well
        assert want[key] == value, (name, key, want[key], value)
    for key, value in want.items():          # every field of LocusLaunch
        assert int(got[key]) == value, (name, key, got[key], value)
    made = [t for t in got["queries"].split("; ") if t]
    assert made == q, (name, made, q)
    if queries is not None:
        assert made == queries, (name, made)


@pytest.mark.parametrize("name", sorted(CASES))
def test_decisions(dumped, name):
    check_case(dumped[name], name)


def test_queries_are_made_only_where_the_rules_say(dumped):
    q = {name: dumped[name]["queries"].split("; ") for name in CASES}
    assert not any(t.startswith("allow") for t in q["A"])
    assert q["C_511"][0] == "allow value 1 5 98304" and q["C_511_denied"][0] == "allow value 1 5 98304"
    assert not any(t.startswith("allow value") for t in q["C_512"])
    assert [t for t in q["D_459"] if t.startswith("allow grad ")] == ["allow grad 153600"]
    assert not any(" grad " in t + " " for t in q["F"])                       # neither allowed nor asked for its occupancy
    assert [t for t in q["H_between"] if "grad2" in t][0] == "allow grad2 3 98304"
    lds2 = int(dumped["H_between"]["grad2_lds"])
    assert 65537 <= lds2 <= 98304 and int(dumped["H_too_large"]["grad2_lds"]) > 98304
    assert not any("grad2" in t for t in q["H_too_large"] + q["H_not_built"] + q["B_eigenbasis_0"])
    assert q["lik_above_64k"][0] == "allow lik 153600" and not any("lik" in t for t in q["lik_too_large"])


def test_nsplit_and_layout(dumped):
    answers = dumped["A"]["answers"]
    assert answers[:len(NSPLIT)] == ["nsplit %d %d %d -> %d" % t for t in NSPLIT]
    assert answers[len(NSPLIT):] == ["layout %d %d %d %d -> %d %d %d %d %d total %d" % (t + o) for t, o in LAYOUT]
    for (items, nn, a, b), o in LAYOUT:      # the layout from its description: lnl | sum | dexch[6] | dlogt[nn]? | d2logt[nn]?
        sizes = [items, items, 6 * items, nn * items * a, nn * items * b]
        assert list(o[:5]) == [sum(sizes[:k]) for k in range(5)] and o[5] == sum(sizes)


def test_call_sizes(dumped):
    """Candidates per chunk (of a million) and tape bytes of either gradient kernel: 1 GiB of eigen-systems [36] and matrices
    [nnodes][16] for the value kernel, 4 GiB of the same plus branch tables [nnodes][12] for the gradient; one tape per resident
    workgroup (here one per CU) of 4 x 128 doubles per slot."""
    for name, nn in (("A", 31), ("lik_too_large", 4799)):
        got = dumped[name]
        assert int(got["value_chunk"]) == min(10 ** 6, (1 << 30) // (8 * (16 * nn + 36))), name
        assert int(got["grad2_chunk"]) == min(10 ** 6, (1 << 32) // (8 * (36 + 28 * nn))), name
    assert int(dumped["A"]["grad_tape_bytes"]) == CUS * (14 + 3) * 4 * 128 * 8
    assert int(dumped["A"]["grad2_tape_bytes"]) == CUS * 14 * 4 * 128 * 8


def test_dump_program_under_sanitizers(tmp_path):
    """Every case once more through the decision code under AddressSanitizer and UBSan (a stand-alone executable)."""
    exe = build_dump(tmp_path, extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name in sorted(CASES):
        check_case(run_dump(exe, CASES[name]), name)


def test_sources_keep_the_decisions_in_one_place():
    """No environment and no HIP in the decision header; the stage-1 unit reads no environment either; the two knobs are plan
    knobs; the gradient's output layout is summed in the header alone."""
    header = open(os.path.join(CSRC, "locus_launch_plan.hpp")).read()
    assert "getenv" not in header and "hip/" not in header
    assert "getenv" not in open(os.path.join(CSRC, "locus_driver.hip")).read()
    knobs = open(os.path.join(CSRC, "site_launch_plan.hpp")).read()
    names = knobs[knobs.index("kPlanKnobNames"):knobs.index("set_plan_knob")]
    assert '"TPHIP_VALUE_COLS"' in names and '"TPHIP_VALUE_EIGENBASIS"' in names
    assert "8 * items" in header
    for name in os.listdir(CSRC):
        text = open(os.path.join(CSRC, name)).read()
        if name.endswith(".hip"):
            assert "8 + (" not in text and "8 * items" not in text, name
            assert "TPHIP_VALUE_COLS" not in text and "TPHIP_VALUE_EIGENBASIS" not in text, name

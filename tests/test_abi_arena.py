"""tests/abi_arena.py on CPU tensors with planted faults: fake "calls" written in numpy that do what a wrong kernel or driver
would -- a byte before an output, a byte after it, a byte past the workspace size they were told, a result that depends on what
the workspace held -- and the carve rules themselves.  If one of them went unseen, tests/test_gpu_abi_contract.py could not
fail for it either."""
import numpy as np
import torch

import abi_arena
from abi_arena import GUARD, PATTERN, Arena

N = 37   # elements of the toy arrays: odd, so that no array ends on a round address


def _arena(aligned=True, ws_stated=None):
    a = Arena(abi_arena.room([(torch.float64, (N,)), (torch.float64, (N,)), (torch.uint8, (N,)), 1000]))
    x = a.carve("x", torch.float64, (N,), "in", aligned=aligned)
    y = a.carve("y", torch.float64, (N,), "out", aligned=aligned)
    f = a.carve("flag", torch.uint8, (N,), "out", aligned=aligned)
    ws = a.carve("ws", torch.uint8, (1000,), "ws", aligned=aligned, stated_bytes=ws_stated)
    x.copy_(torch.arange(N, dtype=torch.float64))
    return a, x, y, f, ws


def _raw(a):
    return a.buf.numpy()   # the arena's bytes, shared with the tensor


def _good_call(a, ws_bytes):
    """y = 2 x through the workspace, flag = 1: writes its scratch before it reads it, stays inside what it was given."""
    raw, e = _raw(a), a.entries
    x = raw[e["x"].offset:e["x"].offset + 8 * N].view(np.float64)
    scratch = raw[e["ws"].offset:e["ws"].offset + ws_bytes][:8 * N].view(np.float64)
    scratch[:] = x
    raw[e["y"].offset:e["y"].offset + 8 * N].view(np.float64)[:] = 2.0 * scratch
    raw[e["flag"].offset:e["flag"].offset + N] = 1


def test_clean_call_is_clean():
    a, x, y, f, ws = _arena(ws_stated=800)
    assert a.check() == [] and a.holds_pattern("y") and a.holds_pattern("flag")
    _good_call(a, 800)
    print("guard bytes watched: %d" % a.guard_bytes)
    assert a.check() == []
    assert a.guard_bytes >= 5 * GUARD + 200
    assert np.array_equal(y.numpy(), 2.0 * np.arange(N)) and np.all(f.numpy() == 1) and not a.holds_pattern("y")


def test_byte_before_an_output_is_seen():
    a, x, y, f, ws = _arena()
    _good_call(a, 1000)
    _raw(a)[a.entries["flag"].offset - 1] = 0
    found = dict(a.check())
    print(found)
    assert found["flag"] == -1


def test_byte_after_an_output_is_seen():
    a, x, y, f, ws = _arena()
    _good_call(a, 1000)
    e = a.entries["flag"]
    _raw(a)[e.offset + e.nbytes] = 0
    found = dict(a.check())
    print(found)
    assert found["flag"] == N
    # ... and at the far end of the band, and a write of the pattern's own complement only
    a2, *_ = _arena()
    e = a2.entries["y"]
    _raw(a2)[e.offset + e.nbytes + GUARD - 1] = PATTERN ^ 0xFF
    assert dict(a2.check())["y"] == e.nbytes + GUARD - 1


def test_byte_past_the_stated_workspace_size_is_seen():
    a, x, y, f, ws = _arena(ws_stated=800)
    _good_call(a, 800)
    assert a.check() == []
    _raw(a)[a.entries["ws"].offset + 800] = 7   # inside the allocation, beyond what the call was told
    found = a.check()
    print(found)
    assert found == [("ws", 800)]
    # the last byte the call may use is not watched
    b, *_ = _arena(ws_stated=800)
    _raw(b)[b.entries["ws"].offset + 799] = 7
    assert b.check() == []


def test_result_that_depends_on_workspace_content_is_seen():
    def leaky_call(a):
        """accumulates into a workspace counter it never reset"""
        raw, e = _raw(a), a.entries
        counter = raw[e["ws"].offset:e["ws"].offset + 8].view(np.int64)
        counter += 3
        raw[e["y"].offset:e["y"].offset + 8 * N].view(np.float64)[:] = float(counter[0] & 0xFF)

    results, clean = [], []
    for byte in (0x00, 0xFF, PATTERN):
        a, x, y, f, ws = _arena()
        a.fill("ws", byte)
        leaky_call(a)
        results.append(y.clone())
        b, xb, yb, fb, wsb = _arena()
        b.fill("ws", byte)
        _good_call(b, 1000)
        clean.append(yb.clone())
        assert a.check() == [] and b.check() == []   # (neither left its arrays: only the bits can tell)
    assert not abi_arena.same_bits(results[0], results[1]) and not abi_arena.same_bits(results[0], results[2])
    assert abi_arena.same_bits(clean[0], clean[1]) and abi_arena.same_bits(clean[0], clean[2])
    # same_bits tells NaN payloads and signed zeros apart, and equal NaNs are equal
    nan = np.array([np.nan, 0.0])
    other = nan.copy()
    other.view(np.uint64)[0] ^= 1
    assert abi_arena.same_bits(nan, nan.copy()) and not abi_arena.same_bits(nan, other)
    assert not abi_arena.same_bits(np.array([0.0]), np.array([-0.0]))


def test_natural_alignment_residues():
    a = Arena(abi_arena.room([(torch.float64, (N,))] * 12))
    want = {torch.int16: 2, torch.int32: 4, torch.float64: 8, torch.int64: 8}
    for k, (dtype, r) in enumerate(want.items()):
        for rep in range(2):   # (whatever came before it)
            t = a.carve("n%d_%d" % (k, rep), dtype, (N,), "in", aligned=False)
            assert t.data_ptr() % 16 == r and t.dtype == dtype and t.is_contiguous() and t.numel() == N
            assert a.address("n%d_%d" % (k, rep)) == t.data_ptr()
    for rep in range(2):
        t = a.carve("byte%d" % rep, torch.uint8, (N,), "in", aligned=False)
        assert t.data_ptr() % 2 == 1
    t = a.carve("al", torch.uint8, (N,), "out", aligned=True)
    assert t.data_ptr() % 256 == 0
    t = a.carve("ws16", torch.uint8, (100,), "ws", address_mod=(32, 16))   # 16-byte aligned and no better
    assert t.data_ptr() % 32 == 16
    t = a.carve("ws_off", torch.uint8, (100,), "ws", address_mod=(256, 1))  # one byte off an aligned address
    assert t.data_ptr() % 256 == 1
    assert a.check() == []
    # the bands of neighbours do not overlap an array: filling every array leaves every band alone
    for name in a.entries:
        a.fill(name, 0)
    assert a.check() == []
    starts = sorted((e.offset, e.nbytes) for e in a.entries.values())
    assert starts[0][0] >= GUARD and all(b[0] - (p[0] + p[1]) >= GUARD for p, b in zip(starts, starts[1:]))
    assert a.buf.numel() - (starts[-1][0] + starts[-1][1]) >= GUARD

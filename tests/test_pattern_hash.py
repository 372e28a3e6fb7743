"""tests/pattern_hash_emulation.py on the CPU: the restated packings and hash, and the two collision finders the GPU tests of
tests/test_gpu_pattern_collisions.py rely on -- distinct columns, equal key / hash under the restatement, no zero nibble,
and the same pair for the same seed."""
import functools

import numpy as np
import pytest

import pattern_hash_emulation as ph

KEY_SEED, FULL_SEED, TREE_SEED = 1, 2, 5


@functools.lru_cache(maxsize=None)
def _tips(ntaxa, workdir):
    from tapir_amd import synth
    root, names = synth.yule_tree(ntaxa, TREE_SEED)
    pin = synth.plan_inputs(root, names)
    return tuple(ph.tip_order(pin["parent"], pin["blen"], pin["leaf"], ntaxa, workdir))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("tree_program"))


def _hash_by_hand(words):
    """The hash in Python integers, one column."""
    h = 0x243F6A8885A308D3
    for w in words:
        h = ((h ^ int(w)) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 29
    return h ^ (h >> 32)


def test_packing_and_hash_restatement():
    """Nibble j of word w is tip 8 w + j, code 0 and high bits normalised, missing tips 0; a tip order permutes the rows first;
    the vectorised uint64 hash equals the same steps in exact integers."""
    col = np.array([1, 2, 4, 8, 0, 15, 0x13, 7, 3, 16], np.uint8)           # 0 -> 15, 0x13 -> 3, 16 -> 0 -> 15
    words = ph.pack_words(col)
    assert words.shape == (2, 1) and words.dtype == np.uint64
    assert int(words[0, 0]) == 0x73FF8421 and int(words[1, 0]) == 0xF3
    order = np.arange(10)[::-1]
    rev = ph.pack_words(col, order)
    assert int(rev[0, 0]) == 0x48FF373F and int(rev[1, 0]) == 0x12
    rng = np.random.default_rng(0)
    cols = rng.integers(0, 256, size=(19, 50), dtype=np.uint8)
    perm = rng.permutation(19)
    for order in (None, perm):
        w = ph.pack_words(cols, order)
        got = ph.hash_words(w)
        assert [int(x) for x in got] == [_hash_by_hand(w[:, c]) for c in range(50)]
    assert np.array_equal(ph.compress_key(cols), ph.hash_words(ph.pack_words(cols)) & np.uint64((1 << 40) - 1))
    assert np.array_equal(ph.classify_hash(cols, perm), ph.hash_words(ph.pack_words(cols[perm])))


def test_tip_order_is_a_permutation_of_the_taxa(workdir):
    for ntaxa in (16, 70):
        order = np.array(_tips(ntaxa, workdir))
        assert sorted(order.tolist()) == list(range(ntaxa))
        assert not np.array_equal(order, np.arange(ntaxa))       # the program does not visit the rows in input order


def test_key_collision_finder():
    a, b, key = ph.find_key_collision(16, KEY_SEED)
    assert a.shape == b.shape == (16,) and a.dtype == b.dtype == np.uint8
    assert not np.array_equal(a, b)
    assert a.min() >= 1 and a.max() <= 15 and b.min() >= 1 and b.max() <= 15
    ka, kb = ph.compress_key(a), ph.compress_key(b)
    assert int(ka[0]) == int(kb[0]) == key < (1 << 40)
    assert _hash_by_hand(ph.pack_words(a)[:, 0]) & ((1 << 40) - 1) == key == _hash_by_hand(ph.pack_words(b)[:, 0]) & ((1 << 40) - 1)
    assert _hash_by_hand(ph.pack_words(a)[:, 0]) != _hash_by_hand(ph.pack_words(b)[:, 0])   # a collision of the key, not of hash 1
    a2, b2, key2 = ph.find_key_collision(16, KEY_SEED)
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and key == key2
    with pytest.raises(ValueError):
        ph.find_key_collision(8, KEY_SEED)


@pytest.mark.parametrize("ntaxa", [16, 70])
def test_full_collision_finder(workdir, ntaxa):
    order = np.array(_tips(ntaxa, workdir))
    pairs = ph.full_collisions(order, FULL_SEED)
    assert len(pairs) >= 3
    for a, b, h in pairs:
        assert a.shape == b.shape == (ntaxa,) and not np.array_equal(a, b)
        assert a.min() >= 1 and a.max() <= 15 and b.min() >= 1 and b.max() <= 15
        assert int(ph.classify_hash(a, order)[0]) == int(ph.classify_hash(b, order)[0]) == h
        assert _hash_by_hand(ph.pack_words(a, order)[:, 0]) == h == _hash_by_hand(ph.pack_words(b, order)[:, 0])
        wa, wb = ph.pack_words(a, order)[:, 0], ph.pack_words(b, order)[:, 0]
        assert wa[0] != wb[0] and wa[1] != wb[1] and np.array_equal(wa[2:], wb[2:])   # two words differ, the rest is shared
    a, b, h = ph.find_full_collision(order, FULL_SEED)
    assert np.array_equal(a, pairs[0][0]) and np.array_equal(b, pairs[0][1]) and h == pairs[0][2]
    again = ph.full_collisions(order, FULL_SEED)
    assert len(again) == len(pairs) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
                                            for x, y in zip(pairs, again))
    assert not np.array_equal(ph.find_full_collision(order, FULL_SEED + 1)[0], a)
    with pytest.raises(ValueError):
        ph.find_full_collision(np.arange(15), FULL_SEED)

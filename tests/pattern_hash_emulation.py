"""The column hash of the two de-duplication paths, restated in numpy uint64, and seeded searches for columns that collide
under it -- for tests that must run a hash collision through tphip_compress_columns (pattern_kernels.hpp) and through the
stage-2 de-duplication (dedup_kernels.hpp on classify_kernel's hash, pi_kernels.hpp).

Both kernels pack a column's normalised 4-bit state masks (code 0 reads as 15) eight to a 32-bit word, nibble j of word w =
tip 8 w + j, missing tips of the last word 0, and hash the words in order:

    h = 0x243F6A8885A308D3;  per word: h = (h ^ word) * 0x9E3779B97F4A7C15, h ^= h >> 29;  at the end: h ^= h >> 32

pack_hash_kernel takes the taxa in input order and sorts by (locus, low 40 bits of h); classify_kernel takes the tips in
tree-program order (TreeProgram::cls_steps: the taxa of the TIP ops of the plain stream) and keys its table by all 64 bits.
A column here is a vector of taxon-major state bytes, as the engine's callers pass them."""
import os
import subprocess

import numpy as np

SEED1 = np.uint64(0x243F6A8885A308D3)
MUL1 = np.uint64(0x9E3779B97F4A7C15)
KEY_BITS = 40
KEY_MASK = np.uint64((1 << KEY_BITS) - 1)
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def normalise(states):
    """The 4-bit masks both kernels work on: the low nibble, 0 read as 15."""
    low = np.asarray(states, np.uint8) & 15
    return np.where(low == 0, 15, low).astype(np.uint8)


def pack_words(states, order=None):
    """states [ntaxa] or [ntaxa, n] -> packed words uint64 [nwords, n] (values < 2^32); order: the row of every tip, in the
    order the kernel visits them (None: input order, pack_hash_kernel)."""
    st = normalise(states)
    if st.ndim == 1:
        st = st[:, None]
    if order is not None:
        st = st[np.asarray(order, np.int64)]
    ntips, n = st.shape
    nwords = (ntips + 7) // 8
    words = np.zeros((nwords, n), np.uint64)
    for t in range(ntips):
        words[t // 8] |= st[t].astype(np.uint64) << np.uint64(4 * (t % 8))
    return words


def mix(h, word):
    """One word into the running hash (pat_mix with the first multiplier; uint64 arrays wrap silently)."""
    h = (h ^ word) * MUL1
    return h ^ (h >> np.uint64(29))


def hash_words(words):
    h = np.full(words.shape[1], SEED1, np.uint64)
    for w in words:
        h = mix(h, w)
    return h ^ (h >> np.uint64(32))


def compress_key(states):
    """The hash part of pack_hash_kernel's sort key, per column: the low 40 bits of hash 1 over the input-order words."""
    return hash_words(pack_words(states)) & KEY_MASK


def classify_hash(states, tip_order):
    """classify_kernel's 64-bit hash, per column."""
    return hash_words(pack_words(states, tip_order))


def tip_order(parent, blen, leaf, ntaxa, workdir):
    """The alignment rows of a tree's tips in program order, from tree_program.hpp itself (tests/native/tree_program_dump.cpp,
    built with g++ into `workdir`): the taxa of the TIP_SET / TIP_MUL ops of the plain stream."""
    exe = os.path.join(str(workdir), "tree_program_dump")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(_ROOT, "tapir_amd", "csrc"),
                               os.path.join(_ROOT, "tests", "native", "tree_program_dump.cpp"), "-o", exe])
    parent, blen, leaf = np.asarray(parent), np.asarray(blen, np.float64), np.asarray(leaf)
    text = "%d %d\n" % (ntaxa, len(parent)) + "".join("%d %.17g %d\n" % (parent[i], blen[i], leaf[i]) for i in range(len(parent)))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    ops = [l.split() for l in out if l.startswith("plain")]
    order = [int(taxon) for _, code, taxon, _ in ops if int(code) <= 1]   # TIP_SET = 0, TIP_MUL = 1
    assert sorted(order) == list(range(ntaxa)), "every taxon is a tip of the program exactly once"
    return np.array(order, np.int64)


def _random_masks(rng, shape):
    """Nonzero 4-bit masks that lean towards an ordinary alignment column: a quarter of them a plain A, the rest uniform on
    1..15 (two of 2^19 such words are equal with probability 6e-8: the birthday search keeps its candidates)."""
    cells = rng.integers(1, 16, size=shape, dtype=np.uint8)
    cells[rng.random(shape) < 0.25] = 1
    return cells


def key_collisions(ntaxa, seed, ncand=3_000_000, max_rounds=8):
    """Every pair of distinct columns with equal 40-bit keys among `ncand` seeded random columns (masks uniform on 1..15);
    the birthday count is ncand^2 / 2^41, about 4, so further seeded rounds are drawn until one holds a pair.  Returns a list
    of (a, b, key), a and b uint8 [ntaxa], in the order of the key."""
    if 15.0 ** ntaxa < 2.0 ** (KEY_BITS + 8):
        raise ValueError("too few taxa for distinct columns to fill the 40-bit key space")
    rng = np.random.default_rng(seed)
    for _ in range(max_rounds):
        cols = rng.integers(1, 16, size=(ntaxa, ncand), dtype=np.uint8)
        key = compress_key(cols)
        order = np.argsort(key, kind="stable")
        ks = key[order]
        pairs = []
        for i in np.flatnonzero(ks[1:] == ks[:-1]):
            a, b = cols[:, order[i]].copy(), cols[:, order[i + 1]].copy()
            if not np.array_equal(a, b):
                pairs.append((a, b, int(ks[i])))
        if pairs:
            return pairs
    raise RuntimeError("no 40-bit key collision in %d rounds of %d columns" % (max_rounds, ncand))


def find_key_collision(ntaxa, seed):
    """Two distinct columns (taxon-major state bytes, no zero nibble) that pack_hash_kernel gives the same sort key within
    a locus, and that key's 40 hash bits: (a, b, key)."""
    return key_collisions(ntaxa, seed)[0]


def full_collisions(tip_order, seed, ncand=1 << 19):
    """Pairs of distinct columns with the same 64-bit classify hash on a tree whose tips come in `tip_order` (>= 16 tips).
    Among `ncand` seeded random first words, two whose states after one step, s and s', agree in the high 32 bits are a
    birthday pair over 32 bits (the golden-ratio multiplier spreads the states of nearby words evenly, so there are fewer
    than the ncand^2 / 2^33 = 32 of a random function: 6 to 23 seen); the second words w and w ^ (s ^ s') -- the difference
    fits a word -- then make the states equal after two steps, and every nibble of w is chosen so that neither word has a zero
    nibble.  All further tips are the same in both columns, which keeps the states equal to the end.  Returns a list of
    (a, b, hash), a and b uint8 [ntaxa] taxon-major."""
    tip_order = np.asarray(tip_order, np.int64)
    ntaxa = len(tip_order)
    if ntaxa < 16:
        raise ValueError("the construction needs two full packed words: 16 tips")
    rng = np.random.default_rng(seed)
    first = _random_masks(rng, (8, ncand))
    w1, keep = np.unique(pack_words(first)[0], return_index=True)   # equal first words are no collision
    first = first[:, keep]
    s1 = mix(np.full(len(w1), SEED1, np.uint64), w1)
    top = s1 >> np.uint64(32)
    order = np.argsort(top, kind="stable")
    ts = top[order]
    pairs = []
    for i in np.flatnonzero(ts[1:] == ts[:-1]):
        ia, ib = int(order[i]), int(order[i + 1])
        diff = int(s1[ia] ^ s1[ib])
        assert diff < (1 << 32)
        a, b = np.zeros(ntaxa, np.uint8), np.zeros(ntaxa, np.uint8)
        rest = _random_masks(rng, ntaxa)            # tips 16.. (program order): shared by both columns
        second = _random_masks(rng, 8)
        for j in range(8):
            d = (diff >> (4 * j)) & 15
            n = int(second[j])
            while n == d:                           # n is never 0; n ^ d is 0 only for n = d
                n = int(rng.integers(1, 16))
            a[tip_order[8 + j]], b[tip_order[8 + j]] = n, n ^ d
        a[tip_order[:8]], b[tip_order[:8]] = first[:, ia], first[:, ib]
        a[tip_order[16:]] = b[tip_order[16:]] = rest[16:]
        ha, hb = classify_hash(a, tip_order), classify_hash(b, tip_order)
        assert ha[0] == hb[0]
        pairs.append((a, b, int(ha[0])))
    if not pairs:
        raise RuntimeError("no birthday pair among %d first words" % ncand)
    return pairs


def find_full_collision(tip_order, seed):
    """Two distinct columns (taxon-major state bytes, no zero nibble) with the same 64-bit classify hash: (a, b, hash)."""
    return full_collisions(tip_order, seed)[0]

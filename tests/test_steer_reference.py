"""tests/steermodel.py -- the model the GPU tests of xfg_steer_egress were first
written against -- and the corpus of tests/steercorpus.py against the
reference's own redirect-cpu programs, compiled for the host without
modification (oracle/ref/ref_cpumap_harness.c).  Whatever is
compared, the expected values come from the reference library alone; where the
two differ the reference is right.  All comparisons are exact.

Skipped where the library was not built (no reference tree at build time); the
GPU file beside this one, test_gpu_steer_reference.py, fails instead.
"""
import functools

import numpy as np
import pytest

import steercorpus as S
import steermodel as M
import xftools as X
from test_steer_model import ROWS, WANT

pytestmark = pytest.mark.skipif(not X.have_reference_steer(),
                                reason="oracle/_ref/libref_cpumap.so not built (no reference tree)")

MODES = [M.L4_HASH, M.L4_SPORT, M.L4_DPORT]
assert MODES == [X.STEER_HASH, X.STEER_SPORT, X.STEER_DPORT]
_w256 = np.random.default_rng(256).integers(0, 5, 256).tolist()
_w256[:8] = [4, 4, 4, 4, 0, 1, 2, 3]
# name -> (avail, skip_queue)
AVAILS = {"id1": ([0], 0), "id2": ([0, 1], 1), "id3": ([0, 1, 2], 0), "id7": (list(range(7)), 6),
          "id64": (list(range(64)), 63), "dup5": ([1, 0, 1, 2, 0], 2), "w256": (_w256, 2)}
NFUZZ = 100_000


def model(data, lens, mode, avail, skip):
    got = [M.queue_of_frame(bytes(data[i, :lens[i]]), mode, avail, skip) for i in range(len(lens))]
    return np.array([q for q, _ in got], np.uint32), np.array([r for _, r in got], bool)


def reference(data, lens, mode, avail, skip):
    """(queue, refused) from the reference; its own counters checked on the way."""
    rec = np.zeros(2, np.uint64)
    q, r = X.run_reference_steer(data.reshape(-1), lens, mode, avail, skip, stride=data.shape[1], rec=rec)
    assert rec.tolist() == [len(lens), 0]           # rec.processed == n, rec.issue == 0
    return q, r


def explain(data, lens, got, want):
    bad = np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))
    out = [f"{len(bad)} of {len(lens)} frames differ"]
    for i in bad[:6].tolist():
        out.append(f"frame {i} len {lens[i]} model {got[0][i], got[1][i]} reference {want[0][i], want[1][i]}: "
                   + data[i, :lens[i]].tobytes().hex())
    return "\n".join(out)


# ---- the model equals the reference
@pytest.mark.parametrize("avail", sorted(AVAILS))
@pytest.mark.parametrize("mode", MODES)
def test_model_on_corpus(mode, avail):
    data, lens = S.slots()
    av, skip = AVAILS[avail]
    want = reference(data, lens, mode, av, skip)
    got = model(data, lens, mode, av, skip)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), explain(data, lens, got, want)


@functools.lru_cache(maxsize=None)
def fuzz():
    """NFUZZ frames of tools/xfsynth.c's fuzz generator; three in four get a
    random stack of one to three VLAN tags pushed in behind the addresses."""
    data, lens = X.gen_fuzz(6324, NFUZZ, S.MAXLEN)
    data = data.reshape(NFUZZ, S.MAXLEN)
    rng = np.random.default_rng(6325)
    depth = rng.integers(0, 4, NFUZZ)
    out, olens = data.copy(), lens.copy()
    for k in (1, 2, 3):
        rows = np.flatnonzero(depth == k)
        out[rows, 12 + 4 * k:] = data[rows, 12:S.MAXLEN - 4 * k]
        tags = rng.integers(0, 256, (len(rows), k, 4), dtype=np.uint8)
        tpid = np.array([[0x81, 0x00], [0x88, 0xa8]], np.uint8)[rng.integers(0, 2, (len(rows), k))]
        tags[:, :, :2] = tpid
        out[rows, 12:12 + 4 * k] = tags.reshape(len(rows), 4 * k)
        olens[rows] = np.minimum(lens[rows] + 4 * k, S.MAXLEN)
    out.setflags(write=False)
    olens.setflags(write=False)
    return out, olens


@pytest.mark.parametrize("avail", sorted(AVAILS))
@pytest.mark.parametrize("mode", MODES)
def test_model_on_random_frames(mode, avail):
    data, lens = fuzz()
    av, skip = AVAILS[avail]
    want = reference(data, lens, mode, av, skip)
    got = model(data, lens, mode, av, skip)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), explain(data, lens, got, want)
    if len(av) > 1:
        assert 0 < want[1].sum() < NFUZZ and len(np.unique(want[0][~want[1]])) == len(set(av))


# ---- the hand table of test_steer_model.py, recomputed from the reference
# 65536, 65535 = 3 * 5 * 17 * 257 and 65533 = 13 * 71 * 71 are coprime in pairs
# and their product is past 2^32: two 32-bit keys congruent modulo all three
# are equal.  (nr_cpus is 65536, so an identity table can be that long.)
MODULI = (65536, 65535, 65533)


def test_hand_table_is_what_the_reference_computes():
    assert X.reference_steer().ref_cpumap_nr_cpus() >= max(MODULI)
    names = sorted(WANT)
    data = np.zeros((len(names), S.MAXLEN), np.uint8)
    for i, nm in enumerate(names):
        data[i, :len(ROWS[nm])] = np.frombuffer(ROWS[nm], np.uint8)
    lens = np.array([len(ROWS[nm]) for nm in names], np.uint32)
    for mode in MODES:
        for m in MODULI:
            q, r = reference(data, lens, mode, np.arange(m), 0)
            for i, nm in enumerate(names):
                k = WANT[nm][mode]
                assert (None if r[i] else int(q[i])) == (None if k is None else k % m), (nm, mode, m)


# ---- the corpus cannot quietly turn bland
@pytest.fixture(scope="module")
def keys():
    """Per mode (key mod 65536, refused) of every corpus frame: in SPORT and
    DPORT the key itself."""
    data, lens = S.slots()
    return [reference(data, lens, mode, np.arange(65536), 0) for mode in MODES]


def test_corpus_conditions(keys):
    data, lens = S.slots()
    n = len(lens)
    for mode in MODES:
        k, refused = keys[mode]
        share = refused.mean()
        nonzero = ((k != 0) & ~refused).mean()
        print(f"mode {mode}: refused {share:.3f}, non-zero key {nonzero:.3f}")
        assert 0.05 <= share <= 0.50
        if mode != M.L4_HASH:
            assert nonzero >= 0.20
    q, refused = reference(data, lens, M.L4_HASH, np.arange(64), 0)
    per = np.bincount(q[~refused], minlength=64)
    print("HASH over 64 queues: fewest", per.min(), "most", per.max(), "of", n)
    assert per.min() >= 1


@pytest.mark.parametrize("tag", [t for t in S.TAGS if S.EXPECT[t]])
def test_reference_result_per_tag(keys, tag):
    """Every return statement the three programs can reach is reached, and the
    reference answers there as the tag says (steercorpus.py's docstring)."""
    c = S.corpus()
    sel = c.tag == S.TAGS.index(tag)
    assert sel.sum() >= 8
    what = S.EXPECT[tag]
    for mode in MODES:
        k, refused = keys[mode]
        if what == "refused":
            assert refused[sel].all()
            continue
        assert not refused[sel].any()
        if what == "zero" or (what == "port0" and mode != M.L4_HASH):
            assert (k[sel] == 0).all()
        elif what == "port" and mode != M.L4_HASH:
            built = (c.sport if mode == M.L4_SPORT else c.dport)[sel]
            assert np.array_equal(k[sel], built)
    if what in ("port0", "port"):
        # a whole IP header is hashed: the keys differ
        assert len(np.unique(keys[M.L4_HASH][0][sel])) > sel.sum() // 50 + 2


def test_symmetry_and_one_word_pairs(keys):
    """The addr part: a swapped pair hashes as the pair does; two IPv6 pairs
    that differ in one word hash apart."""
    c = S.corpus()
    sel = np.flatnonzero(c.part == S.PARTS.index("addr"))
    k = keys[M.L4_HASH][0]
    by_flow = {}
    for i in sel.tolist():
        f = c.frames[i]
        l3 = 14 + 4 * sum(f[12 + 4 * j:14 + 4 * j] in (b"\x81\x00", b"\x88\xa8") for j in range(2))
        v4 = f[l3 - 2:l3] == b"\x08\x00"
        a = f[l3 + 12:l3 + 20] if v4 else f[l3 + 8:l3 + 40]
        half = len(a) // 2
        proto = f[l3 + 9] if v4 else f[l3 + 6]
        by_flow.setdefault((proto, frozenset((a[:half], a[half:]))), set()).add(int(k[i]))
    assert len(by_flow) > 30
    assert all(len(v) == 1 for v in by_flow.values())
    # (pairs whose sums wrap to the same word hash alike, rightly: only the
    # one-word pairs, whose sums differ, are asked to hash apart)
    A6 = bytes(range(1, 17))
    for proto in (6, 17):
        one_word = [v for (p, pair), v in by_flow.items() if p == proto and A6 in pair and len(pair) == 2
                    and sum(x != y for x, y in zip(*sorted(pair))) <= 4]
        assert len(one_word) == 4 and len({next(iter(v)) for v in one_word}) == 4


def test_corpus_shape():
    c = S.corpus()
    data, lens = S.slots()
    assert 10_000 <= len(c.frames) <= 20_000 and data.shape == (len(c.frames), S.MAXLEN)
    assert max(map(len, c.frames)) <= S.MAXLEN and all(n <= len(f) for n, f in zip(lens, c.frames))
    assert set(np.unique(c.tag)) == set(range(len(S.TAGS)))
    assert set(np.unique(c.part)) == set(range(len(S.PARTS)))
    # the double-tagged IPv6 frames: TCP and UDP, every length 0 .. len
    # (bytes 64..65 are the destination port: 61 / 62 and 69 / 70 / 81 / 82
    # are the lengths where the answer changes)
    assert len(c.qinq6) > 600
    full = sorted({len(c.frames[i]) for i in c.qinq6})
    assert full == [14 + 8 + 40 + 8 + 6, 14 + 8 + 40 + 20 + 6]
    assert set(lens[c.qinq6].tolist()) == set(range(full[-1] + 1))
    cut = (lens < np.array([len(f) for f in c.frames])).mean()
    assert cut > 0.3

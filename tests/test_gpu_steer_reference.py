"""xfg_steer_egress against the reference's own redirect-cpu programs, compiled
for the host without modification (oracle/ref/ref_cpumap_harness.c, DESIGN.md
§2), over the corpus of tests/steercorpus.py.  Expected values come from
xftools.run_reference_steer alone -- the queue and the refused flag of every
frame -- and a plain numpy grouping of those queues in record order: no call
to tests/steermodel.py.  Every comparison is exact and whole
(test_gpu_steer.check_steer: 0xA5 prefill, every ring, queue_of, counts and the
UMEM).

Reads only oracle/_ref/*.so (built beside the product, never the reference
tree) and fails where they are absent: a skip would hide the whole file.

The UMEM: 256-byte chunks in permuted order, frame starts at headroom 0 / 16 /
32 / 48 by turns, every third address in the unaligned-chunk form; a chunk
holds its frame's uncut bytes, so behind a cut frame lies its own tail, and
random bytes elsewhere.
"""
import functools

import numpy as np
import pytest

import refcorpus as R
import steercorpus as S
import xftools as X
from test_gpu_steer import MODES, OTHERS, PASS, T, check_after_classify, check_steer

pytestmark = pytest.mark.gpu

CHUNK = 256
ADDR48 = np.uint64((1 << 48) - 1)
QUEUE_NONE = 0xff
HASH, SPORT, DPORT = X.STEER_HASH, X.STEER_SPORT, X.STEER_DPORT
assert MODES == [HASH, SPORT, DPORT]
_w256 = np.random.default_rng(256).integers(0, 5, 256).tolist()
_w256[:8] = [4, 4, 4, 4, 0, 1, 2, 3]
W256 = tuple(_w256)


@pytest.fixture(scope="module")
def G():
    assert X.have_reference_steer(), "oracle/_ref/libref_cpumap.so missing: run the build (make -C oracle ref)"
    import xfgpu
    return xfgpu


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


# ---- the corpus in a UMEM (built once, read only)
@functools.lru_cache(maxsize=None)
def umem_of_corpus(seed=11):
    """(umem, addr, start) per corpus frame."""
    frames = S.corpus().frames
    n = len(frames)
    rng = np.random.default_rng(seed)
    nchunks = n + 7
    umem = rng.integers(0, 256, nchunks * CHUNK, dtype=np.uint8)
    i = np.arange(n)
    base = rng.permutation(nchunks)[:n].astype(np.uint64) * np.uint64(CHUNK)
    head = (16 * (i % 4)).astype(np.uint64)
    assert int(head.max()) + S.MAXLEN <= CHUNK
    start = (base + head).astype(np.int64)
    for k, fr in enumerate(frames):
        umem[start[k]:start[k] + len(fr)] = np.frombuffer(fr, np.uint8)
    addr = np.where(i % 3 == 2, base | (head << np.uint64(48)), base + head).astype(np.uint64)
    for a in (umem, addr, start):
        a.setflags(write=False)
    return umem, addr, start


@functools.lru_cache(maxsize=None)
def reference(mode, avail, skip_queue):
    """(queue, refused) of every corpus frame, from the reference."""
    data, lens = S.slots()
    rec = np.zeros(2, np.uint64)
    q, r = X.run_reference_steer(data.reshape(-1), lens, mode, list(avail), skip_queue, stride=S.MAXLEN,
                                 rec=rec)
    assert rec.tolist() == [len(lens), 0]
    return q, r


def grouped(queue, refused, addr, lens, v, nq):
    """The partition of the records by the reference's queues, in record
    order: (tx, fill, counts, queue_of) as check_steer takes them."""
    passed = np.asarray(v) == PASS
    qof = np.where(passed, queue, QUEUE_NONE).astype(np.uint8)
    tx = []
    for q in range(nq):
        m = qof == q
        rec = np.empty((int(m.sum()), 2), np.uint64)
        rec[:, 0], rec[:, 1] = addr[m], lens[m].astype(np.uint64)
        tx.append(rec)
    fill = addr[~passed] & ADDR48
    counts = np.array([len(t) for t in tx] + [len(fill), int(refused[passed].sum())], np.uint64)
    return tx, fill, counts, qof


def run(G, f, fid, v, nq, mode, avail=None, skip_queue=0, **kw):
    """One call over the records fid (corpus indices) with verdicts v."""
    umem, addr, start = umem_of_corpus()
    lens = S.corpus().lens
    queue, refused = reference(mode, tuple(range(nq)) if avail is None else tuple(avail), skip_queue)
    want = grouped(queue[fid], refused[fid], addr[fid], lens[fid], v, nq)
    return check_steer(G, f, umem, addr[fid], start[fid], lens[fid], v, nq, want, mode=mode,
                       avail=None if avail is None else list(avail), skip_queue=skip_queue, **kw)


def n_corpus():
    return len(S.corpus().frames)


@functools.lru_cache(maxsize=None)
def permuted():
    """A permutation of the corpus and verdicts with 60 % PASS."""
    rng = np.random.default_rng(60)
    n = n_corpus()
    fid = rng.permutation(n)
    v = OTHERS[rng.integers(0, len(OTHERS), n)]
    v[rng.random(n) < 0.6] = PASS
    for a in (fid, v):
        a.setflags(write=False)
    return fid, v


def test_corpus_spans_several_tiles():
    assert n_corpus() > 6 * T and n_corpus() % T


# ---- cases 1, 2: corpus order, all PASS
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq", [7, 64])
def test_corpus_order_all_pass(G, filt, nq, mode):
    n = n_corpus()
    counts = run(G, filt, np.arange(n), np.full(n, PASS, np.uint8), nq, mode, skip_queue=nq - 1,
                 kind=["array", "ring"][mode % 2], rot=mode)
    assert 0.05 * n <= counts[nq + 1] <= 0.5 * n
    if mode == HASH and nq == 64:
        assert counts[:64].min() >= 1


# ---- case 3: permuted, 60 % PASS, the weighted avail table
@pytest.mark.parametrize("mode", MODES)
def test_permuted_weighted_avail(G, filt, mode):
    fid, v = permuted()
    run(G, filt, fid, v, 5, mode, avail=W256, skip_queue=2, kind="ring", rot=1)


# ---- case 4: the same with the MAC swap (every frame named once)
def test_permuted_swap_macs(G, filt):
    fid, v = permuted()
    assert len(np.unique(fid)) == len(fid)
    run(G, filt, fid, v, 5, HASH, avail=W256, skip_queue=2, kind="ring", rot=2, flags=G.EGRESS_SWAP_MACS)


# ---- case 5: bytes 64..65, every lane
@pytest.mark.parametrize("mode", [DPORT, SPORT])
def test_double_tagged_ipv6_every_cut(G, filt, mode):
    """Double-tagged IPv6 TCP / UDP frames cut at every length, two tiles and
    7 records of them: the destination port is the separate load at byte 64,
    made where len >= 70 (UDP) / 82 (TCP)."""
    c = S.corpus()
    n = 2 * T + 7
    fid = np.tile(c.qinq6, n // len(c.qinq6) + 1)[:n]
    lens = c.lens[c.qinq6]
    assert {61, 62, 69, 70, 81, 82} <= set(lens.tolist())
    counts = run(G, filt, fid, np.full(n, PASS, np.uint8), 64, mode, skip_queue=63, kind="ring")
    assert np.count_nonzero(counts[:64]) >= 4 and counts[65] > 0


# ---- case 6: classify, then steer by its verdicts, one stream, no sync
def test_classify_then_steer_without_sync(G):
    assert X.have_reference(), "oracle/_ref/libref_*.so missing: run the build (make -C oracle ref)"
    data, lens = S.slots()
    umem, addr, _ = umem_of_corpus()
    rules = R.rules()
    # (the default-allow program: a frame no rule names passes, so that frames
    # parse_eth refuses and frames of every tag are among the steered ones)
    ov, _, _ = X.run_reference("xdpfilt_alw_all", data.reshape(-1), lens, rules, stride=S.MAXLEN)
    assert 0.4 < np.mean(ov == PASS) < 0.8
    nq = 8
    queue, refused = reference(HASH, tuple(range(nq)), 0)
    want = grouped(queue, refused, addr, lens, ov, nq)
    assert want[2][nq + 1] > 100                      # refused frames among them
    f = G.Filter(X.VARIANT_FEATURES["xdpfilt_alw_all"], ndev=1, descs_min_packets=1)
    try:
        f.load_rules(rules)

        def launch(d_u, d_rx, d_v):
            f.classify_descs(d_u.ptr, d_rx.ptr, len(lens), d_v.ptr)
            return d_rx.ptr, None

        check_after_classify(f, (f, umem, addr, lens, None, ov), nq, HASH, launch, want=want)
    finally:
        f.close()

"""xfg_steer_frags_egress against the reference's own redirect-cpu programs,
compiled for the host without modification (oracle/ref/ref_cpumap_harness.c,
DESIGN.md §2).  An XDP program sees only a multi-buffer packet's first buffer,
so the expected queue of a packet is what cpumap_l4_hash / _sport / _dport
return on the head frame: xftools.run_reference_steer over the head frames
alone, then a plain numpy grouping of the records by packet -- no call to
tests/steermodel.py or tests/steerfragmodel.py for a queue (the shared check()
uses steerfragmodel.packets, the head rule, to say which frames the MAC swap
touches).

The frames of tests/steercorpus.py are the heads, each followed by 0-3
continuation records whose chunks hold other corpus frames: a kernel that
steered by a continuation's bytes, or by the packet's concatenated bytes, would
differ.  The corpus's own conditions (5-50 % refused, all 64 queues hit) are
asserted for the reference on these frames by test_gpu_steer_reference.py and
again here.

Reads only oracle/_ref/*.so and fails where they are absent: a skip would hide
the whole file.
"""
import functools

import numpy as np
import pytest

import steercorpus as S
import xftools as X
from test_gpu_steer import MODES, OTHERS, PASS
from test_gpu_steer_frags import check
from test_gpu_steer_reference import ADDR48, W256, reference, umem_of_corpus

pytestmark = pytest.mark.gpu

QUEUE_NONE = 0xff
CONTD = 1
HASH, SPORT, DPORT = X.STEER_HASH, X.STEER_SPORT, X.STEER_DPORT


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


@functools.lru_cache(maxsize=None)
def packets(permute):
    """Every corpus frame the head of one packet with 0-3 continuation records
    naming other corpus frames.  Returns (fid, opts, pkt, head_fid, v): the
    corpus index, option word and packet number of every record, the corpus
    index of every packet's head, and a verdict byte a record (60 % PASS, drawn
    record by record when @permute; all PASS otherwise)."""
    n = len(S.corpus().frames)
    rng = np.random.default_rng(61 + permute)
    head_fid = rng.permutation(n) if permute else np.arange(n)
    extra = rng.integers(0, 4, n)
    pkt = np.repeat(np.arange(n), extra + 1)
    first = np.concatenate([[0], np.cumsum(extra + 1)[:-1]])
    total = len(pkt)
    fid = rng.integers(0, n, total)
    fid[first] = head_fid
    opts = np.full(total, CONTD, np.uint32)
    opts[first + extra] = 0
    opts |= np.where(np.arange(total) % 5 == 4, 1 << 16, 0).astype(np.uint32)
    if permute:
        v = OTHERS[rng.integers(0, len(OTHERS), total)]
        v[rng.random(total) < 0.6] = PASS
        v[v == 0xff] = 3            # (every record live: liveness is test_gpu_steer_frags.py's)
    else:
        v = np.full(total, PASS, np.uint8)
    for a in (fid, opts, pkt, head_fid, v, first):
        a.setflags(write=False)
    return fid, opts, pkt, head_fid, v, first


def grouped(queue, refused, pkt, first, addr, lens, opts, v, nq):
    """The partition of the records by their packets' queues (@queue, @refused:
    the reference's answer a packet), in record order."""
    head_pass = v[first] == PASS
    pq = np.where(head_pass, queue, QUEUE_NONE).astype(np.uint8)
    qof = pq[pkt]
    word1 = lens.astype(np.uint64) | ((opts & CONTD).astype(np.uint64) << np.uint64(32))
    tx = []
    for q in range(nq):
        m = qof == q
        rec = np.empty((int(m.sum()), 2), np.uint64)
        rec[:, 0], rec[:, 1] = addr[m], word1[m]
        tx.append(rec)
    fill = addr[qof == QUEUE_NONE] & ADDR48
    counts = np.array([len(t) for t in tx] + [len(fill), int(refused[head_pass].sum())], np.uint64)
    return tx, fill, counts, qof


def run(G, f, permute, nq, mode, avail=None, skip_queue=0, **kw):
    umem, caddr, cstart = umem_of_corpus()
    clens = S.corpus().lens
    fid, opts, pkt, head_fid, v, first = packets(permute)
    queue, refused = reference(mode, tuple(range(nq)) if avail is None else tuple(avail), skip_queue)
    want = grouped(queue[head_fid], refused[head_fid], pkt, first, caddr[fid], clens[fid], opts, v, nq)
    counts = check(G, f, umem, caddr[fid], cstart[fid], clens[fid], opts, v, nq, want, mode=mode,
                   avail=None if avail is None else list(avail), skip_queue=skip_queue, **kw)
    return counts, refused[head_fid][v[first] == PASS]


def test_continuations_would_steer_elsewhere():
    """What the file relies on: most continuation records, steered by their own
    bytes, would take another queue than their packet's."""
    fid, opts, pkt, head_fid, v, first = packets(1)
    queue, _ = reference(HASH, tuple(range(64)), 63)
    cont = np.ones(len(fid), bool)
    cont[first] = False
    assert cont.sum() > len(head_fid)
    assert np.mean(queue[fid[cont]] != queue[head_fid[pkt[cont]]]) > 0.5


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq", [7, 64])
def test_corpus_heads_all_pass(G, filt, nq, mode):
    counts, ref = run(G, filt, 0, nq, mode, skip_queue=nq - 1, kind=["array", "ring"][mode % 2], rot=mode,
                      flags=G.EGRESS_MULTIBUF)
    n = len(ref)
    assert 0.05 * n <= counts[nq + 1] <= 0.5 * n and int(ref.sum()) == counts[nq + 1]
    if mode == HASH and nq == 64:
        assert counts[:64].min() >= 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq", [7, 64])
def test_permuted_weighted_avail(G, filt, nq, mode):
    avail = tuple(int(a) * (nq - 1) // 4 for a in W256)      # the weighted table, over nq queues
    assert max(avail) == nq - 1
    run(G, filt, 1, nq, mode, avail=avail, skip_queue=2, kind="ring", rot=1)


def test_permuted_swap_macs(G, filt):
    fid, _, _, _, v, first = packets(1)
    heads = fid[first][v[first] == PASS]
    assert len(np.unique(heads)) == len(heads)      # a frame is the head of one packet
    run(G, filt, 1, 7, HASH, avail=tuple(int(a) * 6 // 4 for a in W256), skip_queue=2, kind="ring", rot=2,
        flags=G.EGRESS_SWAP_MACS)

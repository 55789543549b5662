"""xfg_forward_frags_egress against the reference's own xdp-forward program,
compiled for the host without modification (oracle/ref/ref_forward_harness.c,
DESIGN.md §2).  An XDP program sees only a multi-buffer packet's first buffer,
so the expected port, reason and bytes after of a packet are what
xdp_fwd_fib_full gives the head frame: xftools.run_reference_forward over the
head frames alone (test_gpu_forward_reference.corpus_ref), then a plain numpy
grouping of the records by packet -- no call to tests/fwdmodel.py or
tests/fwdfragmodel.py.

The frames of tests/fwdrefcorpus.py are the heads, each the head of one packet
of 1-4 records; the continuation records name corpus frames too (a frame that
is some packet's head is rewritten at most once all the same: only heads are),
so a kernel that followed a continuation's bytes, or decremented them, would
differ in a ring or in the UMEM, which is compared whole.

Reads only oracle/_ref/*.so and fails where they are absent: a skip would hide
the whole file.
"""
import functools

import numpy as np
import pytest

import fwdrefcorpus as F
import xfgpu as B
import xftools as X
from test_gpu_forward_frags import compare, launch
from test_gpu_forward_reference import ADDR48, QUEUE_NONE, REASONS, corpus_ref, umem_after, umem_of_corpus
from test_gpu_steer import OTHERS, PASS

pytestmark = pytest.mark.gpu

CONTD = 1


@pytest.fixture(scope="module")
def G():
    assert X.have_reference_forward(), "oracle/_ref/libref_forward.so missing: run the build (make -C oracle ref)"
    import xfgpu
    return xfgpu


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fibs(G, filt):
    made = {}

    def get(table):
        if table not in made:
            made[table] = G.Fib(filt, F.routes(), F.nexthops(table))
        return made[table]

    yield get
    for fib in made.values():
        fib.free()


@functools.lru_cache(maxsize=None)
def packets(permute):
    """Every corpus frame the head of one packet with 0-3 continuation records
    naming other corpus frames.  Returns (fid, opts, pkt, head_fid, v, first):
    the corpus index, option word and packet number of every record, the corpus
    index of every packet's head, a verdict byte a record (60 % PASS, drawn
    record by record when @permute; all PASS otherwise) and every packet's
    first record."""
    n = len(F.corpus().frames)
    rng = np.random.default_rng(71 + permute)
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
        v[v == 0xff] = 3            # (every record live: liveness is test_gpu_forward_frags.py's)
    else:
        v = np.full(total, PASS, np.uint8)
    for a in (fid, opts, pkt, head_fid, v, first):
        a.setflags(write=False)
    return fid, opts, pkt, head_fid, v, first


def grouped(queue, reason, pkt, first, addr, lens, opts, v, P):
    """The partition of the records by their packets' queues and reasons
    (@queue, @reason: the reference's answer a packet), in record order."""
    head_pass = v[first] == PASS
    qof = np.where(head_pass, queue, QUEUE_NONE).astype(np.uint8)[pkt]
    rof = np.where(head_pass, reason, QUEUE_NONE).astype(np.uint8)[pkt]
    word1 = lens.astype(np.uint64) | ((opts & CONTD).astype(np.uint64) << np.uint64(32))
    tx = []
    for q in range(P + 1):
        m = qof == q
        rec = np.empty((int(m.sum()), 2), np.uint64)
        rec[:, 0], rec[:, 1] = addr[m], word1[m]
        tx.append(rec)
    fill = addr[qof == QUEUE_NONE] & ADDR48
    counts = np.array([len(t) for t in tx] + [len(fill)] +
                      np.bincount(reason[head_pass], minlength=REASONS).tolist(), np.uint64)
    return tx, fill, counts, qof, rof


def run(G, f, fibs, permute, table, kind="array", rot=0):
    ref = corpus_ref(table)
    umem, caddr, cstart, clens = umem_of_corpus()
    fid, opts, pkt, head_fid, v, first = packets(permute)
    P = len(ref.ifx)
    addr, lens = caddr[fid], clens[fid]
    want = grouped(ref.queue[head_fid], ref.reason[head_fid], pkt, first, addr, lens, opts, v, P)
    # the UMEM after: the PASS heads' frames as the reference left them, nothing else
    hv = np.where(v[first] == PASS, PASS, 0).astype(np.uint8)
    want_umem = umem_after(umem, cstart[head_fid], clens[head_fid], ref.after[head_fid], hv)
    got, blank, rings, tx_first = launch(G, f, fibs(table), False, umem, addr, lens, opts, v, ref.ifx, kind, rot,
                                         True, True, True, G.EGRESS_MULTIBUF)
    compare(got, blank, rings, tx_first, want + (want_umem,), len(v), P)
    return want[2]


def test_continuations_would_go_elsewhere():
    """What the file relies on: most continuation records that the program
    would forward by their own bytes would take another queue than their
    packet's."""
    fid, opts, pkt, head_fid, v, first = packets(1)
    ref = corpus_ref(63)
    cont = np.ones(len(fid), bool)
    cont[first] = False
    own, theirs = ref.queue[fid[cont]], ref.queue[head_fid[pkt[cont]]]
    assert cont.sum() > len(head_fid) and (own < 63).mean() > 0.3
    assert np.mean(own[own < 63] != theirs[own < 63]) > 0.5


@pytest.mark.parametrize("table", [8, 63])
def test_corpus_order_all_pass(G, filt, fibs, table):
    c = run(G, filt, fibs, 0, table, kind=["array", "ring"][table % 2], rot=table % 3)
    assert (c[:table + 1] > 0).all() and (c[table + 2:] >= 50).all()


@pytest.mark.parametrize("table", [8, 63])
def test_permuted_60_percent_pass(G, filt, fibs, table):
    c = run(G, filt, fibs, 1, table, kind="ring", rot=1 + table % 3)
    assert (c[:table + 1] > 0).all() and (c[table + 2:] > 0).all()


def test_colliding_port_table(G, filt, fibs):
    c = run(G, filt, fibs, 0, "collide", kind="ring")
    assert (c[:64] > 0).all() and c[65 + B.FWD_NO_PORT] >= 200

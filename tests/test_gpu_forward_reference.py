"""xfg_forward_egress against the reference's own xdp-forward program, compiled
for the host without modification (oracle/ref/ref_forward_harness.c, DESIGN.md
§2), over the corpus of tests/fwdrefcorpus.py.  Expected values come from
xftools.run_reference_forward alone -- the queue, the stage and the bytes after
of every frame -- and a plain numpy grouping of those queues in record order:
no call to tests/fwdmodel.py.  reason_of is the stage's reason, and the corpus
tag's where the program returns before the lookup (include/xdpfilter_gpu.h
decides that split, the program cannot).  Every comparison is exact and whole
(test_gpu_forward.check_forward: 0xA5 prefill, every ring, queue_of, reason_of,
counts and the UMEM).

Reads only oracle/_ref/*.so (built beside the product, never the reference
tree) and fails where they are absent: a skip would hide the whole file.

The UMEM: 128-byte chunks in permuted order, frame starts at headroom 0 / 16 /
32 by turns, every third address in the unaligned-chunk form, random bytes
behind every frame (test_gpu_steer.umem_of_pool).
"""
import functools

import numpy as np
import pytest

import fwdrefcorpus as F
import refcorpus as R
import xfgpu as B                          # (the binding's XFG_FWD_* numbers; the fixture G is the same module)
import xftools as X
from test_gpu_forward import check_forward
from test_gpu_steer import CHUNK, OTHERS, PASS, T, umem_of_pool

pytestmark = pytest.mark.gpu

ADDR48 = np.uint64((1 << 48) - 1)
QUEUE_NONE = 0xff
REASONS = B.FWD_REASONS
# the reason of a stage past the lookup (xftools.FWD_ST_*), and of a corpus tag in front of it
REASON_OF_STAGE = np.array([QUEUE_NONE, B.FWD_NO_ROUTE, B.FWD_NH_RET, B.FWD_FRAG, B.FWD_NO_PORT, B.FWD_OK,
                            B.FWD_V6], np.uint8)
REASON_OF_TAG = {":49": B.FWD_BAD_HDR, ":52": B.FWD_TTL, ":68": B.FWD_V6, ":71": B.FWD_V6, ":82": B.FWD_NOT_IP}
assert T == F.TILE and F.MAXLEN + 32 <= CHUNK


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
    """One FIB a table, built on first use and alive together."""
    made = {}

    def get(table, f=filt):
        if (table, f) not in made:
            made[table, f] = G.Fib(f, F.routes(), F.nexthops(table))
        return made[table, f]

    yield get
    for fib in made.values():
        fib.free()


# ---- the reference's answers (computed once, read only)
class Ref:
    def __init__(self, data, lens, table, tags=None):
        """Per frame: queue, reason and the bytes after (u8[n, 64], the part of
        a frame the program can write), from the reference alone."""
        ifx = F.ifindexes(table)
        q, stage, after, _ = X.run_reference_forward(data.reshape(-1), lens, F.routes(), F.nexthops(table), ifx,
                                                     stride=data.shape[1])
        reason = REASON_OF_STAGE[stage]
        early = np.flatnonzero(stage == X.FWD_ST_EARLY)
        assert tags is not None or not len(early)
        if len(early):
            reason[early] = [REASON_OF_TAG[F.TAGS[t]] for t in tags[early]]
        w = after.shape[1]
        assert ((q < len(ifx)) == (stage == X.FWD_ST_REDIRECT)).all()
        # what the program did not forward it did not touch
        assert (after[stage != X.FWD_ST_REDIRECT] == data[stage != X.FWD_ST_REDIRECT][:, :w]).all()
        self.ifx, self.queue, self.reason, self.after = ifx, q.astype(np.uint8), reason, after
        for a in (self.queue, self.reason, self.after):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def corpus_ref(table):
    data, lens = F.slots()
    return Ref(data, lens, table, F.corpus().tag)


@functools.lru_cache(maxsize=None)
def umem_of_corpus():
    out = umem_of_pool(F.corpus().frames, 11)
    for a in out:
        a.setflags(write=False)
    return out


def grouped(queue, reason, addr, lens, v, P):
    """The partition of the records by the reference's queues, in record
    order: (tx, fill, counts, queue_of, reason_of) as check_forward takes them."""
    passed = np.asarray(v) == PASS
    qof = np.where(passed, queue, QUEUE_NONE).astype(np.uint8)
    rof = np.where(passed, reason, QUEUE_NONE).astype(np.uint8)
    tx = []
    for q in range(P + 1):
        m = qof == q
        rec = np.empty((int(m.sum()), 2), np.uint64)
        rec[:, 0], rec[:, 1] = addr[m], lens[m].astype(np.uint64)
        tx.append(rec)
    fill = addr[~passed] & ADDR48
    counts = np.array([len(t) for t in tx] + [len(fill)] +
                      np.bincount(rof[passed], minlength=REASONS).tolist(), np.uint64)
    return tx, fill, counts, qof, rof


def umem_after(umem, start, lens, after, v):
    """The UMEM when the call has run: the PASS records' frames as the
    reference left them."""
    want = umem.copy()
    rows = np.flatnonzero(np.asarray(v) == PASS)
    w = after.shape[1]
    cols = np.arange(w)
    at = start[rows][:, None] + cols
    keep = cols[None, :] < lens[rows][:, None]
    want[at[keep]] = after[rows][keep]
    return want


def run(G, f, fib, ref, umem_set, fid, v, **kw):
    """One call over the records fid (distinct indices into the frames ref and
    umem_set describe) with verdicts v."""
    umem, paddr, pstart, plens = umem_set
    assert len(np.unique(fid)) == len(fid)
    addr, lens, start = paddr[fid], plens[fid], pstart[fid]
    P = len(ref.ifx)
    want = grouped(ref.queue[fid], ref.reason[fid], addr, lens, v, P)
    want_umem = umem_after(umem, start, lens, ref.after[fid], v)
    return check_forward(G, f, fib, umem, addr, lens, v, ref.ifx, want + (want_umem,), **kw)


def n_corpus():
    return len(F.corpus().frames)


def test_corpus_spans_several_tiles():
    assert n_corpus() > 4 * T and n_corpus() % T


# ---- case 1: corpus order, all PASS
@pytest.mark.parametrize("table", [1, 8, 63])
def test_corpus_order_all_pass(G, filt, fibs, table):
    n = n_corpus()
    k = [1, 8, 63].index(table)
    c = run(G, filt, fibs(table), corpus_ref(table), umem_of_corpus(), np.arange(n), np.full(n, PASS, np.uint8),
            kind=["array", "ring"][k % 2], rot=k)
    assert (c[:table + 1] > 0).all() and (c[table + 2:] >= 50).all()


# ---- case 2: permuted, about 60 % PASS, rings that wrap
@pytest.mark.parametrize("table", [1, 8, 63])
def test_permuted_wrapping_rings(G, filt, fibs, table):
    fid, v = F.permuted()
    c = run(G, filt, fibs(table), corpus_ref(table), umem_of_corpus(), fid, v, kind="ring", rot=1 + table % 3)
    assert (c[:table + 1] > 0).all() and (c[table + 2:] >= 50).all()


# ---- case 3: the colliding port table
def test_colliding_port_table(G, filt, fibs):
    """63 ports in hash slots 126 and 127: probe chains of up to 62 that wrap
    through slot 0; an absent ifindex that walks the whole chain, one that
    finds its slot empty."""
    n = n_corpus()
    ref = corpus_ref("collide")
    dist = np.array(F.probe_distances(ref.ifx))
    assert (dist[ref.queue[ref.queue < 63]] >= 40).sum() >= 50
    c = run(G, filt, fibs("collide"), ref, umem_of_corpus(), np.arange(n), np.full(n, PASS, np.uint8), kind="ring")
    assert (c[:64] > 0).all() and c[65 + B.FWD_NO_PORT] >= 200    # XFG_FWD_NO_PORT: both absent ifindexes


# ---- case 4: every stored check value
def test_every_check_value(G, filt, fibs):
    """65,536 routed frames, 32 tiles: frame k stores check k (as the
    little-endian load sees it) under k % 5 tags, TTL 2 + k % 254: both carry
    cases of ip_decrease_ttl() at every position the rewrite's selects have."""
    data, lens = F.check_slots()
    ref = Ref(data, lens, 8)
    assert (ref.queue < 8).all() and len(lens) == 32 * T
    pool = [data[i, :lens[i]].tobytes() for i in range(len(lens))]
    n = len(lens)
    c = run(G, filt, fibs(8), ref, umem_of_pool(pool, 12), np.arange(n), np.full(n, PASS, np.uint8), kind="ring",
            rot=2)
    assert c[10 + B.FWD_OK] == n


# ---- case 5: more tiles than workgroups
def test_more_tiles_than_the_grid(G, filt, fibs):
    """The tile loop's second and later tickets: copies of the corpus's UMEM
    block, a chunk of its own for every record, records in a seeded
    permutation with about 60 % PASS.  Everything expected is numpy over the
    per-frame reference answers."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 4 * ncu * T + T + 13
    assert (n + T - 1) // T > 4 * ncu
    ref = corpus_ref(8)
    block, paddr, pstart, plens = umem_of_corpus()
    nc, nchunks = n_corpus(), len(block) // CHUNK
    copies = (n + nc - 1) // nc
    rng = np.random.default_rng(5)
    g = rng.permutation(copies * nc)[:n]                      # record i: corpus frame g % nc of copy g // nc
    fid, copy = g % nc, (g // nc).astype(np.uint64)
    v = OTHERS[rng.integers(0, len(OTHERS), n)]
    v[rng.random(n) < 0.6] = PASS
    umem = np.tile(block, copies)
    addr = paddr[fid] + copy * np.uint64(len(block))          # (the offset form keeps its high bits)
    lens = plens[fid]
    want = grouped(ref.queue[fid], ref.reason[fid], addr, lens, v, 8)
    # the UMEM after, chunk by chunk: a PASS record's chunk as the reference left it in the block
    block_after = umem_after(block, pstart, plens, ref.after, np.full(nc, PASS, np.uint8)).reshape(nchunks, CHUNK)
    want_umem = umem.reshape(copies * nchunks, CHUNK).copy()
    passed = v == PASS
    chunk = pstart[fid][passed] // CHUNK
    want_umem[chunk + copy[passed].astype(np.int64) * nchunks] = block_after[chunk]
    c = check_forward(G, filt, fibs(8), umem, addr, lens, v, ref.ifx, want + (want_umem.reshape(-1),))
    assert (c[:9] > 0).all() and (c[10:] > 0).all()


# ---- case 6: classify, then forward by its verdicts, one stream, no sync
def test_classify_then_forward_without_sync(G, fibs):
    assert X.have_reference(), "oracle/_ref/libref_*.so missing: run the build (make -C oracle ref)"
    data, lens = F.slots()
    rules = R.rules()
    ov, _, _ = X.run_reference("xdpfilt_alw_all", data.reshape(-1), lens, rules, stride=F.MAXLEN)
    n = len(lens)
    assert 0.3 < np.mean(ov == PASS) < 0.95
    ref = corpus_ref(8)
    f = G.Filter(X.VARIANT_FEATURES["xdpfilt_alw_all"], ndev=1, descs_min_packets=1)
    try:
        f.load_rules(rules)
        fib = fibs(8, f)

        def classify(d_u, d_rx, d_v):
            f.classify_descs(d_u.ptr, d_rx.ptr, n, d_v.ptr)

        try:
            c = run(G, f, fib, ref, umem_of_corpus(), np.arange(n), ov, kind="array", options=False,
                    classify=classify)
        finally:
            fib.free()
        assert c[10] > 500 and np.count_nonzero(c[10:]) >= 8     # (classify drops the cut IPv4 headers)
    finally:
        f.close()

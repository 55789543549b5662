"""Many AF_XDP sockets over one UMEM in one call (xfg_classify_socks,
xfg_socks_egress, xfg_socks.hip).

The sockets' batches lie one after the other in flat order; the layouts of
records per socket are chosen around the places the kernels can go wrong
(empty sockets, boundaries on and inside wave and tile edges, a socket carried
across tiles, the largest table).  Every comparison is exact: the egress model
is tests/sockmodel.py (checked on the CPU against hand-written rows and a plain
walk), the classify reference the CPU oracle over the concatenated frames and a
second context fed socket by socket.  Every output ring is uploaded as 0xA5
bytes and compared whole, so entries that must stay untouched are checked too.
"""
import ctypes as C
import errno
import functools
import os
import re

import numpy as np
import pytest

import xftools as X
from sockmodel import bases, sock_model
from test_gpu_egress import A5, PASS, Rings, batch_of, records, slots, umem_for, verdicts_of
from test_gpu_descs import STRIDE, check_all, umem_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ["random", "all_pass", "no_pass", "tile_last"]


def tile():
    src = open(os.path.join(ROOT, "xdp-tools_amd", "csrc", "xfg_layout.h")).read()
    return int(re.search(r"#define\s+XFG_SOCKS_TILE\s+(\d+)u", src).group(1))


@functools.lru_cache(maxsize=None)
def layouts():
    T = tile()
    many = np.random.default_rng(1024).integers(0, 4, 1024)
    assert {0, 1, 2, 3} == set(many.tolist())
    return {
        "one": (97,),
        "empties": (0, 5, 0, 0, 64, 0),
        "wave_edges": (64,) * 64,                        # a boundary on every wave edge
        "in_wave": (1, 1, 2, 3, 57, 1, 63, 64, 65),      # several inside one wave
        "tile_less": (T - 65, 64),                       # one tile less a record, one tile, ...
        "tile": (T - 64, 64),
        "tile_more": (T - 64, 65),                       # ... and a record: the first look-back
        "tile_edges": (T - 1, 1, T, 1, T + 1),           # on and next to tile edges
        "three_tiles": (2 * T, T + 7),                   # a base across two predecessors
        "carry": (3 * T + 7, 2),                         # one socket across three tiles, one behind it
        "many": tuple(int(c) for c in many),             # the largest table, 0..3 records each
    }


LAYOUTS = ["one", "empties", "wave_edges", "in_wave", "tile_less", "tile", "tile_more", "tile_edges",
           "three_tiles", "carry", "many"]


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


class Case:
    """The sockets of one layout: every socket's three rings side by side in
    three device buffers (Rings of test_gpu_egress a socket: plain arrays, or
    power-of-two rings exactly the batch's size whose firsts wrap mid-batch,
    one of them at 0xfffffff0), the shared fill ring, verdicts and counts."""

    def __init__(self, f, counts, kind, batch=None, no_tx=(), no_fill=()):
        self.f, self.counts = f, np.asarray(counts, np.int64)
        self.S, self.n = len(counts), int(self.counts.sum())
        self.base = bases(counts)
        self.rings = [Rings(int(c), kind, rot=s) for s, c in enumerate(counts)]
        self.off = np.zeros((self.S + 1, 3), np.int64)
        self.off[1:] = np.cumsum([r.entries for r in self.rings], axis=0)
        self.addr, self.lens, self.opts = batch or batch_of(self.n)
        self.has_tx = np.array([s not in no_tx for s in range(self.S)])
        self.has_fill = np.array([s not in no_fill for s in range(self.S)])
        self.shared = Rings(self.n, kind, rot=1)
        rec = records(self.addr, self.lens, self.opts)
        self.rx_h = np.full((self.off[-1, 0], 2), A5, np.uint64)
        for s in range(self.S):
            b, c = self.base[s], int(self.counts[s])
            self.rx_h[self.off[s, 0] + self.at(s, 0, c)] = rec[b:b + c]
        self.tx_h = np.full((self.off[-1, 1], 2), A5, np.uint64)
        self.fill_h = np.full(self.off[-1, 2], A5, np.uint64)
        self.sfill_h = np.full(self.shared.entries[2], A5, np.uint64)
        self.d_rx, self.d_tx = f.alloc(self.rx_h.nbytes), f.alloc(self.tx_h.nbytes)
        self.d_fill, self.d_sfill = f.alloc(self.fill_h.nbytes), f.alloc(self.sfill_h.nbytes)
        self.d_v, self.d_c = f.alloc(max(self.n, 16)), f.alloc(8 * (2 * self.S + 2))
        self.bufs = [self.d_rx, self.d_tx, self.d_fill, self.d_sfill, self.d_v, self.d_c]
        self.d_rx.upload(self.rx_h)

    def at(self, s, which, count):
        r = self.rings[s]
        return slots(r.first[which], count, r.mask[which])

    def table(self, G):
        rows = []
        for s, r in enumerate(self.rings):
            rows.append(dict(
                rx_descs=self.d_rx.ptr + 16 * int(self.off[s, 0]), rx_first=r.first[0], rx_mask=r.mask[0],
                tx_descs=self.d_tx.ptr + 16 * int(self.off[s, 1]) if self.has_tx[s] else None,
                tx_first=r.first[1], tx_mask=r.mask[1],
                fill_addrs=self.d_fill.ptr + 8 * int(self.off[s, 2]) if self.has_fill[s] else None,
                fill_first=r.first[2], fill_mask=r.mask[2], count=int(self.counts[s])))
        return G.sock_table(rows)

    def reset_outputs(self):
        self.d_tx.upload(self.tx_h)
        self.d_fill.upload(self.fill_h)
        self.d_sfill.upload(self.sfill_h)
        self.d_c.upload(np.full(2 * self.S + 2, A5, np.uint64))

    def egress(self, G, shared, flags=0, umem_ptr=None, stream=None, table=None):
        self.f.socks_egress(table or self.table(G), self.d_v.ptr, self.d_c.ptr, nsocks=self.S,
                            fill_ptr=self.d_sfill.ptr if shared else None,
                            fill_first=self.shared.first[2], fill_mask=self.shared.mask[2],
                            umem_ptr=umem_ptr, flags=flags, stream=stream)

    def check(self, v, shared):
        """Counts and every ring whole against the model."""
        tx, fill, out = sock_model(self.counts, self.addr, self.lens, v, self.has_tx, self.has_fill,
                                   shared)
        want_tx, want_fill, want_sfill = self.tx_h.copy(), self.fill_h.copy(), self.sfill_h.copy()
        for s in range(self.S):
            want_tx[self.off[s, 1] + self.at(s, 1, len(tx[s]))] = tx[s]
            if not shared:
                want_fill[self.off[s, 2] + self.at(s, 2, len(fill[s]))] = fill[s]
        if shared:
            want_sfill[slots(self.shared.first[2], len(fill), self.shared.mask[2])] = fill
        got = self.d_c.download(np.zeros(2 * self.S + 2, np.uint64))
        np.testing.assert_array_equal(got, out)
        np.testing.assert_array_equal(self.d_tx.download(np.zeros_like(self.tx_h)), want_tx)
        np.testing.assert_array_equal(self.d_fill.download(np.zeros_like(self.fill_h)), want_fill)
        np.testing.assert_array_equal(self.d_sfill.download(np.zeros_like(self.sfill_h)), want_sfill)
        return tx, fill, out

    def free(self):
        for b in self.bufs:
            b.free()


def run_egress(G, f, counts, pattern, kind, shared, **kw):
    c = Case(f, counts, kind, **kw)
    try:
        v = verdicts_of(c.n, pattern)
        if c.n:
            c.d_v.upload(v)
        c.reset_outputs()
        c.egress(G, shared)
        f.sync()
        return c.check(v, shared)
    finally:
        c.free()


# ---- 1: the segmented partition: layouts x verdict patterns x ring forms x fill modes
@pytest.mark.parametrize("shared", [False, True], ids=["own_fill", "shared_fill"])
@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_partition(G, filt, layout, pattern, kind, shared):
    run_egress(G, filt, layouts()[layout], pattern, kind, shared)


@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_one_socket_equals_ring_egress(G, filt, pattern, kind):
    """One socket: the rings and counts xfg_ring_egress writes, byte for byte."""
    f, n = filt, layouts()["one"][0]
    c = Case(f, [n], kind)
    try:
        v = verdicts_of(n, pattern)
        c.d_v.upload(v)
        c.reset_outputs()
        c.egress(G, shared=False)
        f.sync()
        mine = [d.download(np.zeros(d.nbytes, np.uint8)) for d in (c.d_tx, c.d_fill)]
        counts = c.d_c.download(np.zeros(4, np.uint64))
        assert counts[:2].tolist() == counts[2:].tolist()
        c.reset_outputs()
        r = c.rings[0]
        f.ring_egress(c.d_rx.ptr, n, c.d_v.ptr, c.d_c.ptr, tx_ptr=c.d_tx.ptr, fill_ptr=c.d_fill.ptr,
                      rx_first=r.first[0], rx_mask=r.mask[0], tx_first=r.first[1], tx_mask=r.mask[1],
                      fill_first=r.first[2], fill_mask=r.mask[2])
        f.sync()
        for d, m in zip((c.d_tx, c.d_fill), mine):
            np.testing.assert_array_equal(d.download(np.zeros(d.nbytes, np.uint8)), m)
        assert c.d_c.download(np.zeros(2, np.uint64)).tolist() == counts[:2].tolist()
    finally:
        c.free()


# ---- 2: sockets without a TX ring, without a fill ring; the MAC swap
@pytest.mark.parametrize("shared", [False, True], ids=["own_fill", "shared_fill"])
@pytest.mark.parametrize("pattern", ["random", "all_pass"])
def test_sockets_without_a_tx_ring(G, filt, pattern, shared):
    """tx_descs == NULL: the socket sends nothing, its chunks go to the fill side."""
    _, _, out = run_egress(G, filt, layouts()["in_wave"], pattern, "ring", shared, no_tx=(0, 4, 7))
    assert out[2 * 4] == 0 and out[2 * 4 + 1] == 57


@pytest.mark.parametrize("pattern", ["random", "no_pass"])
def test_sockets_without_a_fill_ring(G, filt, pattern):
    """fill_addrs == NULL in per-socket mode: none written, still counted."""
    _, fill, out = run_egress(G, filt, layouts()["in_wave"], pattern, "ring", False,
                              no_fill=(1, 4, 8))
    assert len(fill[4]) == 0 and out[2 * 4 + 1] > 0


@pytest.mark.parametrize("shared", [False, True], ids=["own_fill", "shared_fill"])
def test_swap_macs(G, filt, shared):
    f, counts = filt, layouts()["in_wave"]
    n = sum(counts)
    umem, addr, start = umem_for(n)
    _, lens, opts = batch_of(n)
    c = Case(f, counts, "ring", batch=(addr, lens, opts), no_tx=(4,))
    d_u = f.alloc(umem.nbytes)
    try:
        v = verdicts_of(n, "random")
        c.d_v.upload(v)
        d_u.upload(umem)
        c.reset_outputs()
        c.egress(G, shared, flags=G.EGRESS_SWAP_MACS, umem_ptr=d_u.ptr)
        f.sync()
        c.check(v, shared)
        sent = (v == PASS) & c.has_tx[np.repeat(np.arange(c.S), c.counts)]
        assert 0 < sent.sum() < (v == PASS).sum()
        want = umem.copy()
        at = start[sent][:, None] + np.arange(12)
        want[at] = umem[at][:, [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]]
        np.testing.assert_array_equal(d_u.download(np.zeros_like(umem)), want)
    finally:
        c.free()
        d_u.free()


# ---- 3: the argument checks that need a device
def test_too_many_sockets_and_an_empty_round(G, filt):
    f = filt
    c = Case(f, [0, 0, 0], "array")
    try:
        tab = G.sock_table([dict(rx_descs=c.d_rx.ptr, count=1)] * 1025)
        for call in (lambda: f.classify_socks(c.d_rx.ptr, tab, c.d_v.ptr, nsocks=1025),
                     lambda: f.socks_egress(tab, c.d_v.ptr, c.d_c.ptr, nsocks=1025)):
            with pytest.raises(OSError) as e:
                call()
            assert e.value.errno == errno.EINVAL
        # no record at all: zero counts, nothing launched, no statistic changed
        before = f.stats()
        c.reset_outputs()
        f.classify_socks(None, c.table(G), None)
        c.egress(G, shared=False)
        c.egress(G, shared=True)
        f.sync()
        c.check(np.zeros(0, np.uint8), shared=False)
        assert c.d_c.download(np.zeros(8, np.uint64)).tolist() == [0] * 8
        np.testing.assert_array_equal(f.stats(), before)
    finally:
        c.free()


# ---- 4: classification: real frames scattered over the sockets
@pytest.fixture(scope="module")
def frames():
    """A small mixed rule set and fuzz frames for the largest layout in a UMEM
    (read only); the oracle's results for a prefix of n frames, computed once
    a size."""
    rules, pool = X.random_rules(77, n4=200, n6=80, ne=24, nports=40)
    most = max(sum(c) for c in layouts().values())
    data, lens = X.gen_fuzz(31, most, STRIDE, rules, pool)
    umem, addr = umem_of(data, lens, STRIDE, seed=9)
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]

    @functools.lru_cache(maxsize=None)
    def oracle(n):
        return X.run_oracle(feats, data.reshape(-1)[:n * STRIDE], lens[:n], rules, stride=STRIDE)

    assert {0, 1, 2} <= set(oracle(most)[0].tolist())      # all three verdicts
    return rules, feats, umem, addr, lens, oracle


@pytest.mark.parametrize("layout", LAYOUTS)
def test_classify(G, frames, layout):
    rules, feats, umem, addr, lens, oracle = frames
    counts = layouts()[layout]
    n = sum(counts)
    ov, orules, ost = oracle(n)
    batch = (addr[:n], lens[:n], np.zeros(n, np.uint32))
    f = G.Filter(feats, ndev=1, descs_min_packets=1)
    g = G.Filter(feats, ndev=1, descs_min_packets=1)
    f.load_rules(rules)
    g.load_rules(rules)
    c, cg = Case(f, counts, "ring", batch=batch), Case(g, counts, "ring", batch=batch)
    d_u, d_ug, d_flat = f.alloc(umem.nbytes), g.alloc(umem.nbytes), f.alloc(16 * n)
    try:
        d_u.upload(umem)
        d_ug.upload(umem)
        d_flat.upload(np.full((n, 2), A5, np.uint64))
        f.classify_socks(d_u.ptr, c.table(G), c.d_v.ptr, flat_ptr=d_flat.ptr)
        f.sync()
        assert f.last_path() == G.Filter.PATH_PIPELINE
        v = c.d_v.download(np.zeros(n, np.uint8))
        check_all(G, f, rules, ov, orules, ost, v)          # the oracle over the concatenation
        # the flat array: the sockets' records one after the other, a finished plain array
        np.testing.assert_array_equal(d_flat.download(np.zeros((n, 2), np.uint64)), records(*batch))
        # a second context, socket by socket
        for s, r in enumerate(cg.rings):
            g.classify_descs(d_ug.ptr, cg.d_rx.ptr + 16 * int(cg.off[s, 0]), int(counts[s]),
                             cg.d_v.ptr + int(cg.base[s]), first=r.first[0], mask=r.mask[0])
        g.sync()
        np.testing.assert_array_equal(cg.d_v.download(np.zeros(n, np.uint8)), v)
        np.testing.assert_array_equal(g.stats(), f.stats())
        r = rules.prepared()
        for m, keys in ((G.MAP_IPV4, r.v4_keys), (G.MAP_IPV6, r.v6_keys), (G.MAP_ETHERNET, r.eth_keys),
                        (G.MAP_PORTS, np.arange(65536, dtype=np.uint32))):
            np.testing.assert_array_equal(g.values_of(m, keys), f.values_of(m, keys))
    finally:
        for b in (d_u, d_ug, d_flat):
            b.free()
        c.free()
        cg.free()
        f.close()
        g.close()


def test_classify_into_library_scratch_below_the_threshold(G, frames):
    """No flat array: library scratch; the default descs_min_packets sends a
    batch this small to the general kernel, as for xfg_classify_descs."""
    rules, feats, umem, addr, lens, oracle = frames
    counts = layouts()["tile_edges"]
    n = sum(counts)
    ov, orules, ost = oracle(n)
    f = G.Filter(feats, ndev=1)
    f.load_rules(rules)
    c = Case(f, counts, "array", batch=(addr[:n], lens[:n], np.zeros(n, np.uint32)))
    d_u = f.alloc(umem.nbytes)
    try:
        d_u.upload(umem)
        f.classify_socks(d_u.ptr, c.table(G), c.d_v.ptr)
        f.sync()
        assert f.last_path() == G.Filter.PATH_GENERAL
        check_all(G, f, rules, ov, orules, ost, c.d_v.download(np.zeros(n, np.uint8)))
    finally:
        d_u.free()
        c.free()
        f.close()


# ---- 5: stream order and the socket table's lifetime
@pytest.mark.parametrize("shared", [False, True], ids=["own_fill", "shared_fill"])
def test_rounds_on_a_stream_with_the_table_overwritten(G, frames, shared):
    """Classify then egress, round after round on one non-default stream with
    no host synchronisation, the host socket table overwritten the moment each
    call returns (more rounds than the library has staging slots)."""
    import torch
    rules, feats, umem, addr, lens, oracle = frames
    counts = layouts()["carry"]
    n = sum(counts)
    ov, orules, ost = oracle(n)
    rounds = 10
    f = G.Filter(feats, ndev=1, descs_min_packets=1)
    f.load_rules(rules)
    c = Case(f, counts, "ring", batch=(addr[:n], lens[:n], np.zeros(n, np.uint32)))
    d_u = f.alloc(umem.nbytes)
    try:
        d_u.upload(umem)
        c.d_v.upload(np.full(n, 0xA5, np.uint8))
        c.reset_outputs()
        f.sync()
        stream = torch.cuda.Stream()
        tab = c.table(G)
        good = bytes(tab)
        for _ in range(rounds):
            C.memmove(tab, good, len(good))
            f.classify_socks(d_u.ptr, tab, c.d_v.ptr, nsocks=c.S, stream=stream.cuda_stream)
            C.memset(tab, 0xFF, C.sizeof(tab))          # the table is the caller's again
            C.memmove(tab, good, len(good))
            c.egress(G, shared, stream=stream.cuda_stream, table=tab)
            C.memset(tab, 0xFF, C.sizeof(tab))
        stream.synchronize()
        f.sync()
        np.testing.assert_array_equal(c.d_v.download(np.zeros(n, np.uint8)), ov)
        c.check(ov, shared)
        want = ost.copy()
        want *= np.uint64(rounds)
        np.testing.assert_array_equal(f.stats(), want)
    finally:
        d_u.free()
        c.free()
        f.close()

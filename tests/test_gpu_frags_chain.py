"""A chained stage over multi-buffer batches on the device:
xfg_classify_descs_frags_chain (the record pass and the segment pass, the
selected packets' head records classified as a plain descriptor array, their
verdicts spread over the packets' records; xfg_frags_chain.hip).

The model is tests/fragchainmodel.py (checked on the CPU against hand-written
rows and a record-at-a-time walk, test_frags_chain_abi.py); the verdicts, rule
counters and stats expected of a stage are the CPU oracle's over the selected
packets' head records alone, in their order.  Every comparison is exact, and
every buffer the call writes is uploaded as 0xA5 bytes and compared whole, so
what must stay untouched is checked too.  The records sit in a ring whose u32
index wraps inside the batch, over a UMEM whose every third address is in the
unaligned-chunk form."""
import errno
import functools

import numpy as np
import pytest

import fragchainmodel as M
import xftools as X
from capfragmodel import CONTD, VERDICT_NONE
from test_gpu_chain import (ABORTED, DROP, MASK, MIXED, NFRAMES, PASS, PATTERNS, Bufs, Source, opened,
                            ring_around, traffic, verdicts_in)
from test_gpu_descs import STRIDE, check_all, layout_const

pytestmark = pytest.mark.gpu

A5 = np.uint64(0xA5A5A5A5A5A5A5A5)
A5_32 = 0xA5A5A5A5
ADDR48 = np.uint64(2**48 - 1)
DNY_ALL = X.VARIANT_FEATURES["xdpfilt_dny_all"]
WRAP = 0xfffffff0


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@functools.lru_cache(maxsize=None)
def T():
    t = layout_const("XFG_FRAGS_CHAIN_TILE")
    assert t == 2048
    return t


def sizes():
    t = T()
    return [1, 2, 63, 64, 65, t - 1, t, t + 1, 3 * t + 5]


# ---- the packets' shapes: XDP_PKT_CONTD of every record, and the records whose byte is 0xff
SHAPES = ["single", "three", "random", "heads_at", "long", "cut", "no_eop"]


def random_cont(rng, n, most=5):
    """Packets of 1..most records: 1 on every record but a packet's last."""
    ends = np.cumsum(rng.integers(1, most + 1, n + 1)) - 1
    c = np.ones(n, np.uint32)
    c[ends[ends < n]] = 0
    return c


@functools.lru_cache(maxsize=None)
def shape(n, name):
    t = T()
    rng = np.random.default_rng(1000 * n + SHAPES.index(name))
    c = np.zeros(n, np.uint32)
    dead = np.zeros(n, bool)
    if name == "three":
        c[:] = 1
        c[2::3] = 0                       # (n no multiple of 3: the last packet has no end)
    elif name == "random":
        c = random_cont(rng, n)
    elif name == "heads_at":
        # a packet of three records before the first of each pair, a single record, three records
        for h in (63, 255, t - 1):
            c[max(h - 3, 0):max(h - 1, 0)] = 1
            c[h + 1:h + 3] = 1
        c = c[:n].copy()
    elif name == "long":
        c[5:5 + 2 * t + 6] = 1            # 2t+7 records from record 5 (fewer records: no end)
    elif name == "cut":
        c = random_cont(rng, n)
        eop = c == 0
        head = np.concatenate([[True], eop[:-1]])
        at = np.flatnonzero(head)
        at = at[rng.random(len(at)) < 0.15]
        dead[at[at > 0] - 1] = True       # directly before a head
        dead[at[at + 1 < n] + 1] = True   # and directly after one
    elif name == "no_eop":
        c = random_cont(rng, n)
        p = n // 2
        c[max(p - 3, 0):p] = 1            # a live run into a byte that is not live
        if n > 1:
            dead[p] = True
        c[max(n - 2, 0):] = 1             # and one into the end of the batch
    opts = c | np.where(np.arange(n) % 7 == 3, 6, 0).astype(np.uint32)
    for a in (opts, dead):
        a.setflags(write=False)
    return opts, dead


def verdict_bytes(n, pattern, dead):
    v = verdicts_in(n, pattern).copy()
    v[dead] = VERDICT_NONE
    return v


def frag_source(dev, opts, first=WRAP, src=None):
    """test_gpu_chain's ring Source with XDP_PKT_CONTD from @opts on its
    records; record i is traffic frame src[i]."""
    n = len(opts)
    s = Source(dev, n, "ring", np.arange(n) % NFRAMES if src is None else src)
    s.records[:, 1] |= opts.astype(np.uint64) << np.uint64(32)
    descs, s.first, s.mask = ring_around(s.records, first)
    s.d_descs.upload(descs)
    return s


def frags_chain(f, s, v_ptr, mask, idx_ptr=None, stream=None):
    return f.classify_descs_frags_chain(s.d_base.ptr, s.d_descs.ptr, s.n, v_ptr, chain_mask=mask,
                                        idx_ptr=idx_ptr, first=s.first, mask=s.mask, stream=stream)


def run_stage(f, opts, v_in, mask, v_off, with_idx, first=WRAP):
    """One call over verdict bytes at offset @v_off of their allocation;
    checks the counts, idx, every verdict byte and the guard bytes around both
    against the model.  Returns the traffic frames of the selected heads."""
    ov = traffic()[5]
    n = len(opts)
    dev = Bufs(f)
    try:
        s = frag_source(dev, opts, first)
        buf = np.full(n + 7, 0xA5, np.uint8)
        buf[v_off:v_off + n] = v_in
        d_v = dev(n + 7, buf)
        d_i = dev(4 * n + 4, np.full(n + 1, A5_32, np.uint32))
        counts = frags_chain(f, s, d_v.ptr + v_off, mask, d_i.ptr if with_idx else None)
        f.sync()
        got_v, got_i = d_v.download(np.zeros(n + 7, np.uint8)), d_i.download(np.zeros(n + 1, np.uint32))
    finally:
        dev.free()
    idx, ends, want_counts = M.frags_chain_model(opts, v_in, mask)
    print(f"n {n} v_off {v_off} idx {with_idx} counts {counts} want {want_counts}")
    assert counts == want_counts
    want_i = np.full(n + 1, A5_32, np.uint32)
    if with_idx:
        want_i[:len(idx)] = idx
    np.testing.assert_array_equal(got_i, want_i)
    buf[v_off:v_off + n] = M.merge(v_in, idx, ends, ov[s.src[idx]])
    np.testing.assert_array_equal(got_v, buf)
    return s.src[idx]


class Expect:
    """The oracle's rule values and stats over the heads a context has
    classified so far, call after call."""

    def __init__(self, feats, rules):
        self.feats, self.rules0 = feats, rules
        self.orules, self.ost = rules.prepared(), np.zeros((5, 2), np.uint64)
        self.frames = 0

    def add(self, frames):
        _, data, lens, _, _, _ = traffic()
        if len(frames):
            _, self.orules, self.ost = X.run_oracle(self.feats, data, lens[frames], self.orules,
                                                    offsets=frames.astype(np.uint64) * np.uint64(STRIDE),
                                                    stats=self.ost.copy())
            self.frames += len(frames)

    def check(self, G, f):
        check_all(G, f, self.rules0, None, self.orules, self.ost)
        assert int(self.ost[:, 0].sum()) == self.frames


# ---- 1: shapes x verdict patterns x sizes
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", SHAPES)
def test_shapes_and_patterns(G, name, pattern):
    rules = traffic()[0]
    f = opened(G, DNY_ALL, rules)
    want = Expect(DNY_ALL, rules)
    try:
        for k, n in enumerate(sizes()):
            opts, dead = shape(n, name)
            v_in = verdict_bytes(n, pattern, dead)
            want.add(run_stage(f, opts, v_in, MASK, k % 4, k % 2 == 0))
        want.check(G, f)
    finally:
        f.close()


def test_the_shapes_are_what_they_say():
    t = T()
    n = 3 * t + 5
    ones = np.full(n, PASS, np.uint8)
    idx, ends, counts = M.frags_chain_model(shape(n, "heads_at")[0], ones, MASK)
    assert {63, 64, 255, 256, t - 1, t} <= set(idx.tolist())
    assert all(ends[idx == h][0] == h for h in (63, 255, t - 1))
    assert all(ends[idx == h][0] == h + 2 for h in (64, 256, t))
    idx, ends, _ = M.frags_chain_model(shape(n, "long")[0], ones, MASK)
    assert (ends - idx + 1).max() == 2 * t + 7 and idx[5] == 5 and ends[5] > 2 * t
    opts, dead = shape(n, "cut")
    assert dead.sum() > 50
    idx, ends, counts = M.frags_chain_model(opts, verdict_bytes(n, "all", dead), MASK)
    assert np.any(dead[idx[idx > 0] - 1]) and np.any(dead[np.minimum(ends + 1, n - 1)])
    opts, dead = shape(n, "no_eop")
    idx, ends, counts = M.frags_chain_model(opts, verdict_bytes(n, "all", dead), MASK)
    assert dead[n // 2] and ends.max() < n - 2 and not np.any((idx < n // 2) & (ends >= n // 2 - 3))
    assert counts[2] >= 6


# ---- 2: single-record packets: xfg_classify_descs_chain
@pytest.mark.parametrize("n", [0, 1], ids=["T+1", "3T+5"])
def test_all_end_of_packet_equals_classify_descs_chain(G, n):
    n = [T() + 1, 3 * T() + 5][n]
    rules = traffic()[0]
    v_in = verdicts_in(n, "mixed").copy()
    v_in[v_in == VERDICT_NONE] = 0x80
    opts = np.where(np.arange(n) % 7 == 3, 6, 0).astype(np.uint32)
    got = []
    for frags in (False, True):
        f = opened(G, DNY_ALL, rules)
        dev = Bufs(f)
        try:
            s = frag_source(dev, opts)
            d_v, d_i = dev(n, v_in), dev(4 * n, np.full(n, A5_32, np.uint32))
            if frags:
                c = frags_chain(f, s, d_v.ptr, MASK, d_i.ptr)
                assert c == (c[0], c[0], n - c[0])
            else:
                c = s.chain(f, d_v.ptr, MASK, d_i.ptr)
            f.sync()
            r = rules.prepared()
            got.append([np.array(c[0]), d_v.download(np.zeros(n, np.uint8)),
                        d_i.download(np.zeros(n, np.uint32)), f.stats(),
                        f.values_of(G.MAP_IPV4, r.v4_keys), f.values_of(G.MAP_PORTS,
                                                                        np.arange(65536, dtype=np.uint32))])
        finally:
            dev.free()
            f.close()
    for x, y in zip(*got):
        np.testing.assert_array_equal(x, y)
    assert 0 < int(got[0][0]) < n and got[0][3].any()


# ---- 3: two stages end to end, then egress and capture
def test_two_stages_then_egress_and_capture(G):
    from fragmodel import frag_model
    from test_gpu_capture_frags import first_difference, offsets_of, reference
    from test_gpu_egress import slots
    from test_gpu_frags import egress_model, frag_batch
    fa, fb = X.VARIANT_FEATURES["xdpfilt_alw_tcp"], DNY_ALL
    n = 3 * T() + 5
    umem, rec, opts, hdata, hlens, rules = frag_batch(fa, n, n, seed=3, trail=True)
    pkt_of, _, c3 = frag_model(opts)
    done = c3[1]
    assert c3[2] > 0
    va, orules_a, ost_a = X.run_oracle(fa, hdata, hlens, rules, stride=STRIDE)
    v1 = va[pkt_of[:done]]
    idx, ends, want_counts = M.frags_chain_model(opts[:done], v1, 1 << PASS)
    assert 0 < want_counts[0] < c3[0] and want_counts[1] > want_counts[0]
    pk = pkt_of[idx].astype(np.uint64)
    vb, orules_b, ost_b = X.run_oracle(fb, hdata, hlens[pkt_of[idx]], rules, offsets=pk * np.uint64(STRIDE))
    assert {DROP, PASS} <= set(vb.tolist())
    want = np.full(n, 0xA5, np.uint8)
    want[:done] = M.merge(v1, idx, ends, vb)
    addr, lens = rec[:, 0], (rec[:, 1] & np.uint64(0xffffffff)).astype(np.uint32)
    descs, first, mask = ring_around(rec, WRAP)
    E, room = 8192, 1 << 21
    assert E >= n
    tx_h, fill_h = np.full((E, 2), A5, np.uint64), np.full(E, A5, np.uint64)
    a, b = opened(G, fa, rules), opened(G, fb, rules)
    dev = Bufs(a)
    try:
        d_u, d_rx, d_v = dev(umem.nbytes + 64, umem), dev(descs.nbytes, descs), dev(n, np.full(n, 0xA5, np.uint8))
        d_tx, d_fill, d_c = dev(tx_h.nbytes, tx_h), dev(fill_h.nbytes, fill_h), dev(16)
        d_out, d_cc = dev(room, np.full(room, 0xA5, np.uint8)), dev(32)
        assert a.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask) == c3
        a.sync()
        counts = b.classify_descs_frags_chain(d_u.ptr, d_rx.ptr, done, d_v.ptr, first=first, mask=mask)
        b.sync()
        assert counts == want_counts
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), want)
        # each program keeps its own statistics: A's are those of all packets, B's of the selected
        check_all(G, a, rules, None, orules_a, ost_a)
        check_all(G, b, rules, None, orules_b, ost_b)
        assert int(ost_b[:, 0].sum()) == want_counts[0] and int(ost_a[:, 0].sum()) == c3[0]
        # the result as the egress and the capture take the earlier stage's
        b.ring_egress(d_rx.ptr, done, d_v.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                      rx_first=first, rx_mask=mask, tx_first=E - 100, tx_mask=E - 1,
                      fill_first=WRAP, fill_mask=E - 1, flags=G.EGRESS_MULTIBUF)
        batch = G.DescBatch(d_u.ptr, d_rx.ptr, first, mask, done)
        cmask = 1 << PASS | 1 << DROP
        b.capture_frags_into(batch, d_v.ptr, cmask, d_out.ptr, room, d_cc.ptr, snaplen=96, ts0=42)
        b.sync()
        ec = d_c.download(np.zeros(2, np.uint64)).tolist()
        got_tx, got_fill = d_tx.download(np.zeros_like(tx_h)), d_fill.download(np.zeros_like(fill_h))
        cc = d_cc.download(np.zeros(3, np.uint64)).tolist()
        got_out = d_out.download(np.zeros(room, np.uint8))
    finally:
        dev.free()
        a.close()
        b.close()
    v = want[:done]
    tx, fill = egress_model(addr[:done], lens[:done], opts[:done], v, True)
    assert 0 < len(tx) < done and ec == [len(tx), len(fill)]
    tx_h[slots(E - 100, len(tx), E - 1)] = tx
    fill_h[slots(WRAP, len(fill), E - 1)] = fill
    np.testing.assert_array_equal(got_tx, tx_h)
    np.testing.assert_array_equal(got_fill, fill_h)
    blocks, L = reference(offsets_of(addr)[:done], lens[:done].astype(np.int64), opts[:done], v, cmask, 96,
                          np.full(done, 42, np.uint64), um=umem)
    assert len(blocks) <= room and cc == [len(L), len(blocks), 0]
    expect = np.full(room, 0xA5, np.uint8)
    expect[:len(blocks)] = blocks
    assert np.array_equal(got_out, expect), first_difference(got_out, expect)


# ---- 4: many sockets
def socket_counts(nsocks):
    t = T()
    if nsocks == 1:
        return [t + 77]
    if nsocks == 3:
        return [t - 3, 0, 70]
    c = np.random.default_rng(64).integers(0, 80, nsocks)
    c[[0, 7, 8, 63]] = 0
    c[20] = t - 5
    return [int(x) for x in c]


@pytest.mark.parametrize("nsocks", [1, 3, 64])
def test_many_sockets(G, nsocks):
    from sockfragmodel import classify_model, egress_model, spread
    from sockmodel import bases
    from test_gpu_socks import Case
    from test_gpu_socks_frags import check_rings
    rules, data, lens, umem, addr, ov = traffic()
    counts = socket_counts(nsocks)
    base = bases(counts)
    n = int(base[-1])
    assert n <= NFRAMES
    rng = np.random.default_rng(nsocks)
    cont = random_cont(rng, n, most=4)
    for s, c in enumerate(counts):       # every second socket ends inside a packet, the others on an end
        if c:
            cont[base[s] + c - 1] = s % 2 == 0
    opts = cont | np.where(np.arange(n) % 5 == 4, 1 << 16, 0).astype(np.uint32)
    done, pkt_of, heads, c3 = classify_model(counts, opts)
    assert c3[2] > 0
    v1 = spread(pkt_of, ov[:n][heads])
    idx, ends, want_counts = M.frags_chain_model(opts, v1, 1 << PASS)
    sock_of = np.repeat(np.arange(nsocks), counts)
    assert 0 < want_counts[0] < c3[0]
    np.testing.assert_array_equal(sock_of[idx], sock_of[ends])          # a packet never spans sockets
    rules_b, _ = X.random_rules(5, n4=50, n6=20, ne=5, nports=10)
    vb, orules_b, ost_b = X.run_oracle(DNY_ALL, data, lens[idx], rules_b,
                                       offsets=idx.astype(np.uint64) * np.uint64(STRIDE))
    want = M.merge(v1, idx, ends, vb)
    np.testing.assert_array_equal(want == VERDICT_NONE, pkt_of == 0xffffffff)   # trailing records stay
    a, b = opened(G, DNY_ALL, rules), opened(G, DNY_ALL, rules_b)
    c = Case(a, counts, "ring", batch=(addr[:n], lens[:n], opts))
    dev = Bufs(a)
    try:
        d_u, d_flat = dev(umem.nbytes, umem), dev(16 * n, np.full((n, 2), A5, np.uint64))
        d_i = dev(4 * n + 4, np.full(n + 1, A5_32, np.uint32))
        c.d_v.upload(np.full(max(n, 16), 0xA5, np.uint8))
        c.reset_outputs()
        a.sync()
        got_done, got_c3 = a.classify_socks_frags(d_u.ptr, c.table(G), c.d_v.ptr, flat_ptr=d_flat.ptr)
        a.sync()
        assert got_c3 == c3
        np.testing.assert_array_equal(c.d_v.download(np.zeros(max(n, 16), np.uint8))[:n], v1)
        before = a.stats()
        got = b.classify_descs_frags_chain(d_u.ptr, d_flat.ptr, n, c.d_v.ptr, idx_ptr=d_i.ptr)
        b.sync()                  # (the egress is the other context's, on its own stream)
        a.socks_frags_egress(c.table(G), c.d_v.ptr, c.d_c.ptr, done=got_done, fill_ptr=None,
                             fill_first=c.shared.first[2], fill_mask=c.shared.mask[2], umem_ptr=d_u.ptr,
                             flags=0)
        a.sync()
        b.sync()
        assert got == want_counts
        np.testing.assert_array_equal(c.d_v.download(np.zeros(max(n, 16), np.uint8))[:n], want)
        want_i = np.full(n + 1, A5_32, np.uint32)
        want_i[:len(idx)] = idx
        np.testing.assert_array_equal(d_i.download(np.zeros(n + 1, np.uint32)), want_i)
        check_all(G, b, rules_b, None, orules_b, ost_b)
        np.testing.assert_array_equal(a.stats(), before)
        tx, fill, out = egress_model(counts, done, addr[:n], lens[:n], opts, want, c.has_tx, c.has_fill, False)
        check_rings(c, tx, fill, out, False)
    finally:
        dev.free()
        c.free()
        a.close()
        b.close()


# ---- 5: ring and pointer edge cases
@pytest.mark.parametrize("first", [WRAP, 0, 0xffffffff], ids=["wrap", "zero", "last"])
def test_unaligned_verdicts_and_idx_pointers(G, first):
    rules = traffic()[0]
    n = T() + 3
    opts, dead = shape(n, "cut")
    v_in = verdict_bytes(n, "random", dead)
    f = opened(G, DNY_ALL, rules)
    want = Expect(DNY_ALL, rules)
    try:
        for v_off in (1, 2, 3):
            for with_idx in (True, False):
                want.add(run_stage(f, opts, v_in, MASK, v_off, with_idx, first))
        # fewer records than a dword, at every alignment
        for m in (1, 2, 3, 5):
            for v_off in (0, 1, 2, 3):
                for name in ("single", "three"):
                    o = shape(m, name)[0]
                    want.add(run_stage(f, o, np.full(m, PASS, np.uint8), MASK, v_off, True, first))
        want.check(G, f)
    finally:
        f.close()


def test_workgroups_take_several_tiles(G):
    """More tiles than the grid's four workgroups a CU: the ticket loop's
    second round in both passes, with a packet over the round's edge."""
    import torch
    rules = traffic()[0]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    t = T()
    n = (4 * ncu + 3) * t + 5
    rng = np.random.default_rng(11)
    opts = random_cont(rng, n)
    opts[t * (4 * ncu - 1):t * (4 * ncu + 1) + 9] = 1      # a packet over two tiles of the second round
    v_in = rng.integers(0, 3, n).astype(np.uint8)
    v_in[rng.random(n) < 0.01] = VERDICT_NONE
    f = opened(G, DNY_ALL, rules)
    want = Expect(DNY_ALL, rules)
    try:
        want.add(run_stage(f, opts, v_in, 1 << PASS, 1, True))
        want.check(G, f)
    finally:
        f.close()


# ---- 6: the kernel the heads run on
def test_kernel_choice(G):
    rules = traffic()[0]
    n = T() + 1
    opts, dead = shape(n, "random")
    v_in = verdict_bytes(n, "alternating", dead)
    got = []
    for kw, path in ((dict(descs_min_packets=1), "PATH_PIPELINE"), ({}, "PATH_GENERAL")):
        f = opened(G, DNY_ALL, rules, **kw)
        want = Expect(DNY_ALL, rules)
        try:
            frames = run_stage(f, opts, v_in, MASK, 0, True)
            assert len(frames) > 100
            assert f.last_path() == getattr(G.Filter, path)
            want.add(frames)
            want.check(G, f)
            got.append(f.stats())
        finally:
            f.close()
    np.testing.assert_array_equal(*got)


# ---- 7: nothing selected
def test_nothing_selected_changes_nothing(G):
    rules = traffic()[0]
    n = T() + 1
    opts, dead = shape(n, "no_eop")
    v_in = verdict_bytes(n, "mixed", dead)
    none = np.full(n, PASS, np.uint8)          # every head selected by its byte, no packet complete
    f = opened(G, DNY_ALL, rules)
    dev = Bufs(f)
    try:
        s = frag_source(dev, opts)
        s_open = frag_source(dev, np.ones(n, np.uint32))
        d_v, d_n = dev(n, v_in), dev(n, none)
        d_i = dev(4 * n, np.full(n, A5_32, np.uint32))
        for mask in (0, 1 << 5 | 1 << 30):
            assert frags_chain(f, s, d_v.ptr, mask, d_i.ptr) == (0, 0, n)
            assert frags_chain(f, s, d_v.ptr, mask, None) == (0, 0, n)
        assert frags_chain(f, s_open, d_n.ptr, MASK, d_i.ptr) == (0, 0, n)
        assert f.classify_descs_frags_chain_timed(s.d_base.ptr, s.d_descs.ptr, n, d_v.ptr, chain_mask=0,
                                                  first=s.first, mask=s.mask) == ((0, 0, n), (0.0, 0.0, 0.0))
        c, ms = f.classify_descs_frags_chain_timed(s.d_base.ptr, s.d_descs.ptr, n, d_v.ptr, chain_mask=1 << 7,
                                                   first=s.first, mask=s.mask)
        assert c == (0, 0, n) and ms[0] > 0 and ms[1:] == (0.0, 0.0)
        f.sync()
        with pytest.raises(OSError) as e:                           # nothing was ever launched
            f.last_path()
        assert e.value.errno == errno.ENOENT
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), v_in)
        np.testing.assert_array_equal(d_n.download(np.zeros(n, np.uint8)), none)
        np.testing.assert_array_equal(d_i.download(np.zeros(n, np.uint32)), np.full(n, A5_32, np.uint32))
        assert not f.stats().any()
        check_all(G, f, rules, None, rules.prepared(), np.zeros((5, 2), np.uint64))
        # ... and after a call that classified: the path stays what that call left
        assert frags_chain(f, s, d_v.ptr, MASK)[0] > 0
        f.sync()
        path, stats = f.last_path(), f.stats()
        assert frags_chain(f, s, d_v.ptr, 0) == (0, 0, n)
        assert frags_chain(f, s_open, d_n.ptr, MASK) == (0, 0, n)
        f.sync()
        assert f.last_path() == path
        np.testing.assert_array_equal(f.stats(), stats)
    finally:
        dev.free()
        f.close()


def test_timed_call_gives_the_same_results(G):
    rules = traffic()[0]
    n = 3 * T() + 5
    opts, dead = shape(n, "random")
    v_in = verdict_bytes(n, "random", dead)
    idx, ends, want_counts = M.frags_chain_model(opts, v_in, 1 << PASS)
    ov = traffic()[5]
    f = opened(G, DNY_ALL, rules)
    want = Expect(DNY_ALL, rules)
    dev = Bufs(f)
    try:
        s = frag_source(dev, opts)
        d_v = dev(n, v_in)
        counts, ms = f.classify_descs_frags_chain_timed(s.d_base.ptr, s.d_descs.ptr, n, d_v.ptr,
                                                        first=s.first, mask=s.mask)
        print("ms", ms)
        assert counts == want_counts and len(ms) == 3 and all(0 < m < 1000 for m in ms)
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)),
                                      M.merge(v_in, idx, ends, ov[s.src[idx]]))
        want.add(s.src[idx])
        want.check(G, f)
    finally:
        dev.free()
        f.close()

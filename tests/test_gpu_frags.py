"""Multi-buffer AF_XDP packets on the device: xfg_classify_descs_frags (head
pass, heads classified, verdicts spread; xfg_frags.hip) and xfg_ring_egress
with XFG_EGRESS_MULTIBUF.

The model of the head pass is fragmodel.frag_model (checked on the CPU against
hand-written rows, test_frags_abi.py); the verdicts, rule counters and stats
expected of a batch are the CPU oracle's over the head records' bytes and
lengths alone.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

import xftools as X
from fragmodel import CONTD, frag_model

pytestmark = pytest.mark.gpu

PASS = 2
A5 = np.uint64(0xA5A5A5A5A5A5A5A5)
ADDR48 = np.uint64(2**48 - 1)
STRIDE, CHUNK = 160, 256


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@functools.lru_cache(maxsize=None)
def T():
    from test_gpu_descs import layout_const
    return layout_const("XFG_FRAGS_TILE")


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


class Bufs:
    """Device buffers freed together."""

    def __init__(self, f):
        self.f, self.held = f, []

    def __call__(self, nbytes, init=None):
        b = self.f.alloc(max(int(nbytes), 16))
        self.held.append(b)
        if init is not None and init.nbytes:
            b.upload(init)
        return b

    def free(self):
        for b in self.held:
            b.free()


def ring(records, kind):
    """The records in a plain array, or in a power-of-two ring whose u32 index
    wraps inside the batch (first = 0xfffffff0); the other entries 0xA5."""
    n = len(records)
    if kind == "array":
        return records if n else np.zeros((1, 2), np.uint64), 0, 0xffffffff
    e = 16
    while e < n + 3:
        e *= 2
    first = 0xfffffff0
    descs = np.full((e, 2), A5, np.uint64)
    descs[(first + np.arange(n)) & 0xffffffff & (e - 1)] = records
    return descs, first, e - 1


# ---- 1: the head pass
PATTERNS = ["all_eop", "no_eop", "alt2", "random", "wave_edge", "tile_edge", "long", "trail1", "trailT3"]


def head_sizes():
    t = T()
    return [0, 1, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 3 * t + 7, 2**20 + 13]


@functools.lru_cache(maxsize=None)
def options_of(n, pattern):
    """u32 options of n records: bit 0 by the pattern, other bits (ignored) on
    some records."""
    t = T()
    rng = np.random.default_rng(100 * n + PATTERNS.index(pattern))
    c = np.zeros(n, np.uint32)
    if pattern == "no_eop":
        c[:] = 1
    elif pattern == "alt2":
        c[0::2] = 1                      # (an odd n ends in a lone continued record)
    elif pattern == "random":
        frags = rng.integers(1, 5, n + 1)
        ends = np.cumsum(frags) - 1
        c[:] = 1
        c[ends[ends < n]] = 0
    elif pattern == "wave_edge":
        c[62:65] = 1                     # one packet over records 62..65
    elif pattern == "tile_edge":
        c[max(t - 2, 0):t + 1] = 1       # ... over t-2..t+1
    elif pattern == "long":
        c[3:3 + 2 * t + 4] = 1           # 2t+5 records from record 3: a whole tile without an end
    elif pattern == "trail1":
        c[n - 1:] = 1
    elif pattern == "trailT3":
        c[max(n - (t + 3), 0):] = 1
    opts = c | np.where(np.arange(n) % 5 == 4, 1 << 16, 0).astype(np.uint32) \
             | np.where(np.arange(n) % 7 == 3, 6, 0).astype(np.uint32)
    opts.setflags(write=False)
    return opts


NCHUNK = 64


def head_records(opts):
    """Records over a 64-chunk UMEM of zero bytes: the heads classify to some
    verdict, the same for every packet of one length."""
    n = len(opts)
    r = np.empty((n, 2), np.uint64)
    r[:, 0] = (np.arange(n) % NCHUNK).astype(np.uint64) * np.uint64(64)
    r[:, 1] = (14 + np.arange(n) % 3).astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    return r


@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", range(13))
def test_head_pass(filt, n, pattern, kind):
    n = head_sizes()[n]
    opts = options_of(n, pattern)
    want_pkt, heads, want_counts = frag_model(opts)
    descs, first, mask = ring(head_records(opts), kind)
    dev = Bufs(filt)
    try:
        d_u = dev(NCHUNK * 64, np.zeros(NCHUNK * 64, np.uint8))
        d_rx = dev(descs.nbytes, descs)
        d_v = dev(n + 3, np.full(n + 3, 0xA5, np.uint8))
        d_p = dev(4 * n + 4, np.full(n + 1, 0xA5A5A5A5, np.uint32))
        # (a verdict buffer at an odd address: the spread's unaligned lead)
        counts = filt.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr + 1, pkt_of_ptr=d_p.ptr,
                                           first=first, mask=mask)
        filt.sync()
        v = d_v.download(np.zeros(n + 3, np.uint8))
        p = d_p.download(np.zeros(n + 1, np.uint32))
    finally:
        dev.free()
    assert counts == want_counts
    assert counts[1] + counts[2] == n
    np.testing.assert_array_equal(p[:n], want_pkt)
    assert p[n] == 0xA5A5A5A5
    done = counts[1]
    assert v[0] == 0xA5
    np.testing.assert_array_equal(v[1 + done:], np.full(n + 2 - done, 0xA5, np.uint8))
    got = v[1:1 + done]
    assert np.all(got <= 2)
    if done:      # every record carries its packet's (its head record's) verdict
        head_at = np.flatnonzero(heads)
        np.testing.assert_array_equal(got, got[head_at[want_pkt[:done]]])


def test_head_pass_workgroups_take_several_tiles(filt):
    """More tiles than the grid's four workgroups a CU (the sizes above stay
    below that on a large device): the ticket loop's second round."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = (4 * ncu + 3) * T() + 5
    rng = np.random.default_rng(11)
    opts = (rng.random(n) < 0.6).astype(np.uint32)
    opts[T() * (4 * ncu - 1):T() * (4 * ncu + 1) + 9] = 1      # a tile of the second round without an end
    want_pkt, _, want_counts = frag_model(opts)
    dev = Bufs(filt)
    try:
        d_u = dev(NCHUNK * 64, np.zeros(NCHUNK * 64, np.uint8))
        d_rx, d_v, d_p = dev(16 * n, head_records(opts)), dev(n), dev(4 * n)
        counts = filt.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, pkt_of_ptr=d_p.ptr)
        filt.sync()
        p = d_p.download(np.zeros(n, np.uint32))
    finally:
        dev.free()
    assert counts == want_counts
    np.testing.assert_array_equal(p, want_pkt)


def test_library_scratch_for_the_packet_indices(filt):
    """pkt_of == NULL: the same verdicts."""
    n = 3 * T() + 7
    opts = options_of(n, "random")
    descs, first, mask = ring(head_records(opts), "array")
    dev = Bufs(filt)
    try:
        d_u = dev(NCHUNK * 64, np.zeros(NCHUNK * 64, np.uint8))
        d_rx, d_p = dev(descs.nbytes, descs), dev(4 * n)
        d_v = [dev(n, np.full(n, 0xA5, np.uint8)) for _ in range(2)]
        c0 = filt.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v[0].ptr, pkt_of_ptr=d_p.ptr)
        c1 = filt.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v[1].ptr)
        filt.sync()
        v = [d.download(np.zeros(n, np.uint8)) for d in d_v]
    finally:
        dev.free()
    assert c0 == c1 == frag_model(opts)[2]
    np.testing.assert_array_equal(v[0], v[1])


# ---- 2: parity with the oracle over the head records
@functools.lru_cache(maxsize=None)
def traffic(npkts):
    rules, pool = X.random_rules(77, n4=200, n6=80, ne=24, nports=40)
    data, lens = X.gen_fuzz(31, npkts, STRIDE, rules, pool)
    for a in (data, lens):
        a.setflags(write=False)
    return rules, data, lens


def hit_frames(feats, rules, data, lens, want=3):
    """Frames of the batch that hit a rule under this program (VERDICT_HIT:
    PASS for a deny program, DROP for an allow one)."""
    m = min(len(lens), 4096)
    v, _, _ = X.run_oracle(feats, data[:m * STRIDE], lens[:m], rules, stride=STRIDE)
    at = np.flatnonzero(v == (PASS if feats & X.FEAT_DENY else 1))[:want]
    assert len(at) == want
    return at


SPECIAL_HEADS = [0, 13, 14, 20, 34, 64]


def frag_batch(feats, npkts, nrec, seed, trail=False):
    """npkts fuzz frames as packets of a head plus 0-3 continuation records,
    cut to the first nrec records (None: all), the last one continued with
    @trail (a trailing incomplete packet, whatever the draw).  A head record holds its frame
    with a head length of its own; every continuation chunk holds a whole frame
    that hits a rule.  Returns (umem, records, opts, head bytes, head lens of
    the complete packets, rules)."""
    rules, data, lens = traffic(npkts)
    rng = np.random.default_rng(seed)
    hits = hit_frames(feats, rules, data, lens)
    slots = data.reshape(npkts, STRIDE)
    nf = rng.integers(0, 4, npkts)
    hl = np.where(nf == 0, lens, rng.integers(0, lens.astype(np.int64) + 1)).astype(np.uint32)
    for j, h in enumerate(SPECIAL_HEADS):
        nf[j] = max(nf[j], 1)
        hl[j] = h
    pkt = np.repeat(np.arange(npkts), nf + 1)
    starts = np.cumsum(nf + 1) - (nf + 1)
    is_head = np.zeros(len(pkt), bool)
    is_head[starts] = True
    last = np.zeros(len(pkt), bool)
    last[starts + nf] = True
    total = len(pkt)
    chunk_of = rng.permutation(total + 7)[:total]
    umem = np.zeros((total + 7, CHUNK), np.uint8)
    r = np.arange(total)
    room = (16 * (r % 3)).astype(np.int64)
    which = hits[rng.integers(0, len(hits), total)]          # a continuation's frame
    src = np.where(is_head, pkt, which)
    for h in (0, 16, 32):
        sel = room == h
        umem[chunk_of[sel], h:h + STRIDE] = slots[src[sel]]
    base = chunk_of.astype(np.uint64) * np.uint64(CHUNK)
    ro = room.astype(np.uint64)
    addr = np.where(r % 3 == 2, base | (ro << np.uint64(48)), base + ro).astype(np.uint64)
    rlen = np.where(is_head, hl[pkt], lens[which]).astype(np.uint64)
    opts = np.where(last, 0, CONTD).astype(np.uint32) | np.where(r % 5 == 4, 1 << 16, 0).astype(np.uint32)
    rec = np.empty((total, 2), np.uint64)
    rec[:, 0] = addr
    rec[:, 1] = rlen | (opts.astype(np.uint64) << np.uint64(32))
    if nrec is not None:
        assert total >= nrec
        rec, opts = rec[:nrec], opts[:nrec]
    if trail:
        rec[-1, 1] |= np.uint64(CONTD << 32)
        opts[-1] |= CONTD
    npk = frag_model(opts)[2][0]
    return umem.reshape(-1), rec, opts, data[:npk * STRIDE], hl[:npk], rules


def check_all(G, f, rules, orules, ost):
    from test_gpu_descs import check_all as chk
    chk(G, f, rules, None, orules, ost)


@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("prog", ["xdpfilt_dny_all", "xdpfilt_alw_tcp", "xdpfilt_dny_eth"])
def test_parity_with_the_oracle(G, prog, kind):
    feats = X.VARIANT_FEATURES[prog]
    n = 1025
    umem, rec, opts, hdata, hlens, rules = frag_batch(feats, n, n, seed=3, trail=True)
    pkt_of, _, want_counts = frag_model(opts)
    assert want_counts[2] > 0 and want_counts[0] == len(hlens)
    ov, orules, ost = X.run_oracle(feats, hdata, hlens, rules, stride=STRIDE)
    ov2, orules2, ost2 = X.run_oracle(feats, hdata, hlens, orules, stride=STRIDE, stats=ost.copy())
    descs, first, mask = ring(rec, kind)
    f = G.Filter(feats, ndev=1)
    f.load_rules(rules)
    dev = Bufs(f)
    try:
        d_u, d_rx = dev(umem.nbytes, umem), dev(descs.nbytes, descs)
        d_v = dev(n, np.full(n, 0xA5, np.uint8))
        counts = f.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask)
        f.sync()
        assert counts == want_counts
        v = d_v.download(np.zeros(n, np.uint8))
        done = counts[1]
        np.testing.assert_array_equal(v[:done], ov[pkt_of[:done]])
        np.testing.assert_array_equal(v[done:], np.full(n - done, 0xA5, np.uint8))
        check_all(G, f, rules, orules, ost)
        # two calls in a row without a read between them: twice the counters
        f2 = G.Filter(feats, ndev=1)
        f2.load_rules(rules)
        try:
            for _ in range(2):
                assert f2.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first,
                                               mask=mask) == want_counts
            f2.sync()
            check_all(G, f2, rules, orules2, ost2)
        finally:
            f2.close()
    finally:
        dev.free()
        f.close()


def test_parity_heads_on_the_pipelined_kernel(G):
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    npkts = 2**17 + 100
    umem, rec, opts, hdata, hlens, rules = frag_batch(feats, npkts, None, seed=4)
    n = len(opts)
    pkt_of, _, want_counts = frag_model(opts)
    assert want_counts == (npkts, n, 0)
    ov, orules, ost = X.run_oracle(feats, hdata, hlens, rules, stride=STRIDE)
    f = G.Filter(feats, ndev=1)
    f.load_rules(rules)
    dev = Bufs(f)
    try:
        d_u, d_rx, d_v, d_p = dev(umem.nbytes, umem), dev(rec.nbytes, rec), dev(n), dev(4 * n)
        counts = f.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, pkt_of_ptr=d_p.ptr)
        f.sync()
        assert counts == want_counts
        assert f.last_path() == G.Filter.PATH_PIPELINE
        np.testing.assert_array_equal(d_p.download(np.zeros(n, np.uint32)), pkt_of)
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), ov[pkt_of])
        check_all(G, f, rules, orules, ost)
    finally:
        dev.free()
        f.close()


def test_no_end_of_packet_changes_nothing(G):
    """Every record continued: nothing classified, no counter, no statistic."""
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    umem, rec, opts, _, _, rules = frag_batch(feats, 1025, 300, seed=3)
    rec = rec.copy()
    rec[:, 1] |= np.uint64(CONTD << 32)
    f = G.Filter(feats, ndev=1)
    f.load_rules(rules)
    dev = Bufs(f)
    try:
        d_u, d_rx = dev(umem.nbytes, umem), dev(rec.nbytes, rec)
        d_v = dev(300, np.full(300, 0xA5, np.uint8))
        assert f.classify_descs_frags(d_u.ptr, d_rx.ptr, 300, d_v.ptr) == (0, 0, 300)
        assert f.classify_descs_frags(d_u.ptr, d_rx.ptr, 0, d_v.ptr) == (0, 0, 0)
        f.sync()
        np.testing.assert_array_equal(d_v.download(np.zeros(300, np.uint8)), np.full(300, 0xA5, np.uint8))
        assert not f.stats().any()
        check_all(G, f, rules, rules.prepared(), np.zeros((5, 2), np.uint64))
    finally:
        dev.free()
        f.close()


# ---- 3: a batch without a continuation bit is xfg_classify_descs' batch
def test_single_buffer_batch_equals_classify_descs(G):
    from test_gpu_descs import ALL_PORTS, ring_of, umem_of
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    rules, data, lens = traffic(4097)
    umem, addr = umem_of(data, lens, STRIDE, seed=5)
    descs, first, mask = ring_of(addr, lens, 8192, 8192 - 777, fill=0xFF)
    n = len(lens)
    got = []
    for frags in (False, True):
        f = G.Filter(feats, ndev=1)
        f.load_rules(rules)
        dev = Bufs(f)
        try:
            d_u, d_rx, d_v = dev(umem.nbytes, umem), dev(descs.nbytes, descs), dev(n)
            if frags:
                assert f.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first,
                                              mask=mask) == (n, n, 0)
            else:
                f.classify_descs(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask)
            f.sync()
            r = rules.prepared()
            got.append([d_v.download(np.zeros(n, np.uint8)), f.stats(),
                        f.values_of(G.MAP_IPV4, r.v4_keys), f.values_of(G.MAP_IPV6, r.v6_keys),
                        f.values_of(G.MAP_ETHERNET, r.eth_keys), f.values_of(G.MAP_PORTS, ALL_PORTS),
                        f.last_path()])
        finally:
            dev.free()
            f.close()
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)
    assert got[0][1].any() and got[0][2].any()


# ---- 4: egress with XFG_EGRESS_MULTIBUF
def egress_model(addr, lens, opts, v, multibuf):
    m = v == PASS
    tx = np.empty((int(m.sum()), 2), np.uint64)
    tx[:, 0] = addr[m]
    keep = (opts[m] & CONTD).astype(np.uint64) if multibuf else np.uint64(0)
    tx[:, 1] = lens[m].astype(np.uint64) | (keep << np.uint64(32))
    return tx, addr[~m] & ADDR48


@functools.lru_cache(maxsize=None)
def egress_case(n):
    """n records of complete packets of 1-4 fragments, a verdict per packet
    spread over its records."""
    from test_gpu_egress import OTHERS
    rng = np.random.default_rng(7000 + n)
    frags = rng.integers(1, 5, n + 1)
    ends = np.cumsum(frags) - 1
    c = np.ones(n, np.uint32)
    c[ends[ends < n]] = 0
    if n:
        c[n - 1] = 0
    opts = c | np.where(np.arange(n) % 5 == 4, 1 << 16, 0).astype(np.uint32)
    pkt_of, heads, counts = frag_model(opts)
    pv = OTHERS[rng.integers(0, len(OTHERS), counts[0])]
    pv[rng.random(counts[0]) < 0.5] = PASS
    v = pv[pkt_of]
    for a in (opts, v, heads):
        a.setflags(write=False)
    return opts, v, heads


@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("n", range(4))
def test_egress_multibuf(G, filt, n, swap, kind):
    from test_gpu_egress import Rings, batch_of, records, slots, umem_for
    n = [1, 65, T() + 1, 3 * T() + 7][n]
    opts, v, heads = egress_case(n)
    umem, addr, start = umem_for(n)
    _, lens, _ = batch_of(n)
    rings = Rings(n, kind, rot=n % 3)
    for flags in (G.EGRESS_MULTIBUF, 0):
        rx_h = np.full((max(rings.entries[0], 1), 2), A5, np.uint64)
        rx_h[slots(rings.first[0], n, rings.mask[0])] = records(addr, lens, opts)
        tx_h = np.full((rings.entries[1], 2), A5, np.uint64)
        fill_h = np.full(rings.entries[2], A5, np.uint64)
        dev = Bufs(filt)
        try:
            d_rx, d_tx, d_fill = dev(rx_h.nbytes, rx_h), dev(tx_h.nbytes, tx_h), dev(fill_h.nbytes, fill_h)
            d_v, d_c, d_u = dev(n, v), dev(16, np.full(2, A5, np.uint64)), dev(umem.nbytes, umem)
            filt.ring_egress(d_rx.ptr, n, d_v.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                             rx_first=rings.first[0], rx_mask=rings.mask[0],
                             tx_first=rings.first[1], tx_mask=rings.mask[1],
                             fill_first=rings.first[2], fill_mask=rings.mask[2], umem_ptr=d_u.ptr,
                             flags=flags | (G.EGRESS_SWAP_MACS if swap else 0))
            filt.sync()
            counts = d_c.download(np.zeros(2, np.uint64)).tolist()
            got_tx, got_fill = d_tx.download(np.zeros_like(tx_h)), d_fill.download(np.zeros_like(fill_h))
            got_umem = d_u.download(np.zeros_like(umem))
        finally:
            dev.free()
        want_tx, want_fill = egress_model(addr, lens, opts, v, bool(flags))
        assert counts == [len(want_tx), len(want_fill)]       # per record, as l2fwd's tx_frags
        tx_h[slots(rings.first[1], len(want_tx), rings.mask[1])] = want_tx
        fill_h[slots(rings.first[2], len(want_fill), rings.mask[2])] = want_fill
        np.testing.assert_array_equal(got_tx, tx_h)
        np.testing.assert_array_equal(got_fill, fill_h)
        if not flags:      # without the flag: options 0 everywhere
            assert not (got_tx[slots(rings.first[1], len(want_tx), rings.mask[1]), 1] >> np.uint64(32)).any()
        want = umem.copy()
        if swap:           # the PASS heads with the flag, every PASS record without it
            sel = (v == PASS) & (heads if flags else True)
            at = start[sel][:, None] + np.arange(12)
            want[at] = umem[at][:, [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]]
        np.testing.assert_array_equal(got_umem, want)


# ---- 5: classify with fragments, then egress, on one stream without a sync between
@pytest.mark.parametrize("where", ["library_stream", "caller_stream"])
def test_classify_frags_then_egress(G, where):
    import torch
    from test_gpu_egress import slots
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    n = 3 * T() + 7
    umem, rec, opts, hdata, hlens, rules = frag_batch(feats, n, n, seed=9)
    rec, opts = rec.copy(), opts.copy()
    rec[n - 2:, 1] |= np.uint64(CONTD << 32)       # a trailing incomplete packet, whatever the draw
    opts[n - 2:] |= CONTD
    pkt_of, heads, want_counts = frag_model(opts)
    npk, done, trail = want_counts
    assert trail >= 2 and npk <= len(hlens)
    ov, _, _ = X.run_oracle(feats, hdata[:npk * STRIDE], hlens[:npk], rules, stride=STRIDE)
    assert 0 < np.count_nonzero(ov == PASS) < npk
    descs, first, mask = ring(rec, "ring")
    stream = torch.cuda.Stream() if where == "caller_stream" else None
    sp = stream.cuda_stream if stream else None
    f = G.Filter(feats, ndev=1)
    f.load_rules(rules)
    dev = Bufs(f)
    E = 8192
    assert E >= n
    tx_h, fill_h = np.full((E, 2), A5, np.uint64), np.full(E, A5, np.uint64)
    try:
        d_u, d_rx, d_v = dev(umem.nbytes, umem), dev(descs.nbytes, descs), dev(n, np.zeros(n, np.uint8))
        d_tx, d_fill, d_c = dev(tx_h.nbytes, tx_h), dev(fill_h.nbytes, fill_h), dev(16)
        f.sync()
        counts = f.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask, stream=sp)
        assert counts == want_counts
        f.ring_egress(d_rx.ptr, counts[1], d_v.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                      rx_first=first, rx_mask=mask, tx_first=E - 100, tx_mask=E - 1,
                      fill_first=0xfffffff0, fill_mask=E - 1, flags=G.EGRESS_MULTIBUF, stream=sp)
        if stream:
            stream.synchronize()
        f.sync()
        ec = d_c.download(np.zeros(2, np.uint64)).tolist()
        got_tx, got_fill = d_tx.download(np.zeros_like(tx_h)), d_fill.download(np.zeros_like(fill_h))
    finally:
        dev.free()
        f.close()
    assert sum(ec) == done                          # TX records plus fill entries: frags_done
    v = ov[pkt_of[:done]]
    addr, lens = rec[:done, 0], (rec[:done, 1] & np.uint64(0xffffffff)).astype(np.uint32)
    want_tx, want_fill = egress_model(addr, lens, opts[:done], v, True)
    assert ec == [len(want_tx), len(want_fill)]
    tx_h[slots(E - 100, len(want_tx), E - 1)] = want_tx
    fill_h[slots(0xfffffff0, len(want_fill), E - 1)] = want_fill
    np.testing.assert_array_equal(got_tx, tx_h)
    np.testing.assert_array_equal(got_fill, fill_h)
    # no packet split between the rings: the TX ring holds whole packets (as
    # many ends as PASS packets, the last record an end), each PASS packet's
    # records adjacent and in order
    tx = got_tx[slots(E - 100, ec[0], E - 1)]
    tx_c = (tx[:, 1] >> np.uint64(32)) & np.uint64(CONTD)
    assert int((tx_c == 0).sum()) == int(np.count_nonzero(ov == PASS)) and tx_c[-1] == 0
    np.testing.assert_array_equal(tx[:, 0], addr[v == PASS])

"""Chained contexts on the device: xfg_classify_chain and
xfg_classify_descs_chain (select pass by verdict, the selected frames
classified as a plain descriptor array, their verdicts scattered back;
xfg_chain.hip).

The model of the select pass is tests/chainmodel.py (checked on the CPU against
a per-frame loop, test_chain_abi.py); the verdicts, rule counters and stats
expected of a stage are the CPU oracle's over the selected frames alone, in
their order.  Every comparison is exact, and every buffer the call writes is
uploaded as 0xA5 bytes and compared whole, so what must stay untouched is
checked too."""
import errno
import functools

import numpy as np
import pytest

import chainmodel as M
import pktbuild as P
import xftools as X
from test_gpu_descs import STRIDE, check_all, layout_const, umem_of

pytestmark = pytest.mark.gpu

ABORTED, DROP, PASS = 0, 1, 2
A5 = np.uint64(0xA5A5A5A5A5A5A5A5)
ADDR48 = np.uint64(2**48 - 1)
DNY_ALL = X.VARIANT_FEATURES["xdpfilt_dny_all"]
# the select tests' chain mask: PASS, 4 and 31 run the program; 3, 32, 0x80, 0xff do not
MASK = 1 << PASS | 1 << 4 | 1 << 31


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@functools.lru_cache(maxsize=None)
def T():
    return layout_const("XFG_CHAIN_TILE")


class Bufs:
    """Device buffers freed together."""

    def __init__(self, f):
        self.f, self.held = f, []

    def __call__(self, nbytes, init=None):
        b = self.f.alloc(max(int(nbytes), 16))
        self.held.append(b)
        if init is not None and init.nbytes:
            b.upload(np.ascontiguousarray(init))
        return b

    def free(self):
        for b in self.held:
            b.free()


def opened(G, feats, rules, **opts):
    f = G.Filter(feats, ndev=1, **opts)
    f.load_rules(rules)
    return f


# ---- the frames every select test shares, and the oracle's verdict for each
NFRAMES = 3 * 2048 + 5


@functools.lru_cache(maxsize=None)
def traffic():
    """Rules, NFRAMES fuzz frames in 160-byte slots, the same frames in a UMEM
    (permuted chunks, headroom, every third address in the unaligned-chunk
    form), and the verdict of xdpfilt_dny_all for each frame (read only)."""
    rules, pool = X.random_rules(77, n4=200, n6=80, ne=24, nports=40)
    data, lens = X.gen_fuzz(31, NFRAMES, STRIDE, rules, pool)
    umem, addr = umem_of(data, lens, STRIDE, seed=5)
    ov, _, _ = X.run_oracle(DNY_ALL, data, lens, rules, stride=STRIDE)
    assert {ABORTED, DROP, PASS} <= set(ov.tolist())
    for a in (data, lens, umem, addr, ov):
        a.setflags(write=False)
    return rules, data, lens, umem, addr, ov


@pytest.fixture(scope="module")
def filt(G):
    f = opened(G, DNY_ALL, traffic()[0])
    yield f
    f.close()


PATTERNS = ["none", "all", "first", "last", "alternating", "random", "mixed"]
MIXED = np.array([ABORTED, DROP, PASS, PASS, 3, 4, 31, 32, 0x80, 0xff], np.uint8)


@functools.lru_cache(maxsize=None)
def verdicts_in(n, pattern):
    """The earlier stage's verdict bytes."""
    rng = np.random.default_rng(100 * n + PATTERNS.index(pattern))
    v = np.full(n, DROP, np.uint8)
    if pattern == "all":
        v[:] = PASS
    elif pattern == "first":
        v[0] = PASS
    elif pattern == "last":
        v[-1] = PASS
    elif pattern == "alternating":
        v[0::2] = PASS
    elif pattern == "random":
        v = rng.integers(0, 3, n).astype(np.uint8)
    elif pattern == "mixed":
        v = MIXED[rng.integers(0, len(MIXED), n)]
    v.setflags(write=False)
    return v


def ring_around(records, first):
    """The records in a power-of-two ring from u32 index @first on; the other
    entries 0xA5."""
    n, e = len(records), 16
    while e < n + 3:
        e *= 2
    descs = np.full((e, 2), A5, np.uint64)
    descs[((first + np.arange(n)) & 0xffffffff) & (e - 1)] = records
    return descs, first, e - 1


FORMS = ["stride", "offsets_u16", "offsets_u32", "ring"]


class Source:
    """n frames of traffic() in one source form, uploaded; frame i of the
    batch is traffic frame src[i]."""

    def __init__(self, dev, n, form, src=None):
        _, data, lens, umem, addr, _ = traffic()
        self.n, self.form = n, form
        self.src = np.arange(n) if src is None else src
        self.lens = lens[self.src]
        if form == "ring":
            rec = np.empty((n, 2), np.uint64)
            rec[:, 0] = addr[self.src]
            rec[:, 1] = self.lens.astype(np.uint64) | (np.arange(n) % 5 == 4).astype(np.uint64) << np.uint64(48)
            self.records = rec
            descs, self.first, self.mask = ring_around(rec, 0xfffffff0)     # wraps past 2^32 inside the batch
            self.d_base, self.d_descs = dev(umem.nbytes, umem), dev(descs.nbytes, descs)
            return
        assert src is None
        self.d_base = dev(n * STRIDE, data[:n * STRIDE])
        self.offsets = None
        if form != "stride":      # the slots named in another order
            self.src = np.random.default_rng(n).permutation(n)
            self.lens = lens[self.src]
            self.offsets = self.src.astype(np.uint64) * np.uint64(STRIDE)
            self.d_offs = dev(8 * n, self.offsets)
        self.u16 = form == "offsets_u16"
        self.d_lens = dev(4 * n, self.lens.astype(np.uint16 if self.u16 else np.uint32))

    def chain(self, f, v_ptr, mask, idx_ptr=None, stream=None):
        if self.form == "ring":
            return f.classify_descs_chain(self.d_base.ptr, self.d_descs.ptr, self.n, v_ptr, chain_mask=mask,
                                          idx_ptr=idx_ptr, first=self.first, mask=self.mask, stream=stream)
        return f.classify_chain(self.d_base.ptr, self.d_lens.ptr, self.n, STRIDE if self.offsets is None else 0,
                                v_ptr, chain_mask=mask, idx_ptr=idx_ptr,
                                offsets_ptr=None if self.offsets is None else self.d_offs.ptr,
                                lens_u16=self.u16, stream=stream)


def run_select(f, n, form, v_in, mask, v_off, with_idx, src=None):
    """One chained call over verdict bytes at offset @v_off of their
    allocation; checks the counts, idx, every verdict byte and the guard
    bytes around both against the model."""
    ov = traffic()[5]
    dev = Bufs(f)
    try:
        s = Source(dev, n, form, src)
        buf = np.full(n + 3, 0xA5, np.uint8)
        buf[v_off:v_off + n] = v_in
        d_v = dev(n + 3, buf)
        d_i = dev(4 * n + 4, np.full(n + 1, 0xA5A5A5A5, np.uint32))
        counts = s.chain(f, d_v.ptr + v_off, mask, d_i.ptr if with_idx else None)
        f.sync()
        got_v, got_i = d_v.download(np.zeros(n + 3, np.uint8)), d_i.download(np.zeros(n + 1, np.uint32))
    finally:
        dev.free()
    idx, want_counts = M.chain_model(v_in, mask)
    assert counts == want_counts
    want_i = np.full(n + 1, 0xA5A5A5A5, np.uint32)
    if with_idx:
        want_i[:len(idx)] = idx
    np.testing.assert_array_equal(got_i, want_i)
    buf[v_off:v_off + n] = M.merge(v_in, idx, ov[s.src[idx]])
    np.testing.assert_array_equal(got_v, buf)


def select_sizes():
    t = T()
    return [1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 5]


# ---- 1: the select pass, the new verdicts in place, the rest untouched
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", range(8))
def test_select_pass(filt, n, pattern, form):
    n = select_sizes()[n]
    assert n <= NFRAMES
    v_in = verdicts_in(n, pattern)
    run_select(filt, n, form, v_in, MASK, 0, True)      # verdicts at offset 0, idx given
    run_select(filt, n, form, v_in, MASK, 1, False)     # at offset 1, idx in library scratch


@pytest.mark.parametrize("form", FORMS)
def test_select_pass_other_pointer_pairs(filt, form):
    n = T() + 1
    run_select(filt, n, form, verdicts_in(n, "mixed"), MASK, 1, True)
    run_select(filt, n, form, verdicts_in(n, "mixed"), MASK, 0, False)


@pytest.mark.parametrize("mask", [1 << 3, 1 << 31 | 1 << 0, 0xffffffff])
def test_select_pass_other_masks(filt, mask):
    n = T() + 1
    run_select(filt, n, "stride", verdicts_in(n, "mixed"), mask, 1, True)


def test_select_pass_workgroups_take_several_tiles(filt):
    """More tiles than the grid's four workgroups a CU (the sizes above stay
    below that on a large device): the ticket loop's second round."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = (4 * ncu + 3) * T() + 5
    v = np.random.default_rng(11).integers(0, 3, n).astype(np.uint8)
    v[T() * (4 * ncu - 1):T() * (4 * ncu + 1) + 9] = DROP      # a tile of the second round with nothing selected
    run_select(filt, n, "ring", v, 1 << PASS, 0, True, src=np.arange(n) % NFRAMES)


# ---- 2: two stages against the oracle
def rule_set(ports=(), v4=(), v6=(), eth=()):
    rs = X.RuleSet()
    for port, flags in ports:
        rs.ports[X.port_key(port)] = np.uint64(flags)
    for name, keys, conv, width in (("v4", v4, P.ip4, 4), ("v6", v6, P.ip6, 16), ("eth", eth, P.mac, 6)):
        k = np.array([list(conv(a)) for a, _ in keys], np.uint8).reshape(-1, width)
        setattr(rs, name + "_keys", k)
        setattr(rs, name + "_vals", np.array([fl for _, fl in keys], np.uint64))
    return rs


V4 = ["10.11.1.1", "10.11.1.2", "10.11.7.7", "192.168.3.9"]
V6 = ["fc00:dead:cafe:1::1", "fc00:dead:cafe:1::2", "fc00:dead:cafe:9::77"]
MACS = ["02:00:00:00:00:0a", "02:00:00:00:00:0b", "02:00:00:00:00:0c"]
PORTS = [53, 123, 4000, 5000]
S, D, TC, U = X.FLAG_SRC, X.FLAG_DST, X.FLAG_TCP, X.FLAG_UDP


@functools.lru_cache(maxsize=None)
def two_stage():
    """Mixed traffic built frame by frame: UDP, TCP, ICMP, ARP and cut-off
    frames over IPv4 and IPv6 (some behind a VLAN tag), 5,003 of them drawn
    from the templates; an allow-list context A for UDP ports, a deny-list
    context B for addresses."""
    rng = np.random.default_rng(2024)
    templates = []
    for v6 in (False, True):
        addrs = V6 if v6 else V4
        for src in addrs:
            for dst in addrs:
                for smac in MACS:
                    for dport in PORTS:
                        for sport in (12345, 123):
                            for l4 in ("udp", "tcp"):
                                seg = P.udp(sport, dport) if l4 == "udp" else P.tcp(sport, dport)
                                proto = 17 if l4 == "udp" else 6
                                l3 = P.ipv6(src, dst, nh=proto, payload=seg) if v6 else \
                                    P.ipv4(src, dst, proto=proto, payload=seg)
                                vl = ((0x8100, 5),) if dport == 5000 and sport == 123 else ()
                                templates.append(P.eth(P.mac(MACS[1]), P.mac(smac), 0x86dd if v6 else 0x0800,
                                                       vlans=vl) + l3)
    templates.append(P.eth(ethertype=0x0806) + P.arp())
    templates.append(P.ping4(V4[0], V4[2]))
    templates.append(P.ping6(V6[0], V6[2]))
    cut = [t[:k] for t in templates[:40] for k in (0, 10, 14, 30, 40)]
    templates += cut
    assert max(len(t) for t in templates) <= STRIDE
    n = 5003
    pick = rng.integers(0, len(templates), n)
    data = np.zeros((n, STRIDE), np.uint8)
    lens = np.zeros(n, np.uint32)
    for i, p in enumerate(pick):
        t = templates[p]
        data[i, :len(t)] = np.frombuffer(t, np.uint8)
        lens[i] = len(t)
    rules_a = rule_set(ports=[(53, D | U), (4000, S | D | U | TC), (123, S | U), (5000, D | TC)])
    rules_b = rule_set(v4=[(V4[0], S), (V4[2], S | D), (V4[3], D)], v6=[(V6[1], D), (V6[2], S)],
                       eth=[(MACS[2], S), (MACS[1], S)])
    data = data.reshape(-1)
    for a in (data, lens):
        a.setflags(write=False)
    return data, lens, rules_a, rules_b


def oracle_stage(feats, data, lens, rules, idx):
    """The oracle over the selected frames alone, in their order."""
    d = M.descs_of_batch(lens, idx, STRIDE)
    return X.run_oracle(feats, data, d[:, 1].astype(np.uint32), rules, offsets=d[:, 0])


@pytest.mark.parametrize("form", ["batch", "descs"])
@pytest.mark.parametrize("mask", [1 << PASS, 1 << PASS | 1 << ABORTED], ids=["PASS", "PASS_ABORTED"])
def test_two_stage_parity(G, mask, form):
    data, lens, rules_a, rules_b = two_stage()
    n = len(lens)
    fa, fb = X.VARIANT_FEATURES["xdpfilt_alw_udp"], DNY_ALL
    va, orules_a, ost_a = X.run_oracle(fa, data, lens, rules_a, stride=STRIDE)
    idx, want_counts = M.chain_model(va, mask)
    vb, orules_b, ost_b = oracle_stage(fb, data, lens, rules_b, idx)
    assert {ABORTED, DROP, PASS} <= set(va.tolist()) and {DROP, PASS} <= set(vb.tolist())
    assert orules_b.v4_vals.max() >> 6 and orules_b.v6_vals.max() >> 6 and orules_b.eth_vals.max() >> 6
    want = M.merge(va, idx, vb)
    a, b = opened(G, fa, rules_a), opened(G, fb, rules_b)
    dev = Bufs(a)
    try:
        d_v = dev(n, np.full(n, 0xA5, np.uint8))
        if form == "batch":
            d_d, d_l = dev(data.nbytes, data), dev(lens.nbytes, lens)
            a.classify(d_d.ptr, d_l.ptr, n, STRIDE, d_v.ptr)
            a.sync()
            counts = b.classify_chain(d_d.ptr, d_l.ptr, n, STRIDE, d_v.ptr, chain_mask=mask)
        else:
            umem, addr = umem_of(data, lens, STRIDE, seed=3)
            rec = np.stack([addr, lens.astype(np.uint64)], axis=1)
            descs, first, rmask = ring_around(rec, 0xfffff000)
            d_u, d_rx = dev(umem.nbytes, umem), dev(descs.nbytes, descs)
            a.classify_descs(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=rmask)
            a.sync()
            counts = b.classify_descs_chain(d_u.ptr, d_rx.ptr, n, d_v.ptr, chain_mask=mask, first=first,
                                            mask=rmask)
        b.sync()
        assert counts == want_counts
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), want)
        # each program keeps its own statistics: A's are those of all frames, B's of the selected
        check_all(G, a, rules_a, None, orules_a, ost_a)
        check_all(G, b, rules_b, None, orules_b, ost_b)
        assert int(ost_b[:, 0].sum()) == len(idx) < n == int(ost_a[:, 0].sum())
    finally:
        dev.free()
        a.close()
        b.close()


# ---- 3: further cases
def results(G, f, rules, d_v, n):
    r = rules.prepared()
    return [d_v.download(np.zeros(n, np.uint8)), f.stats(), f.values_of(G.MAP_IPV4, r.v4_keys),
            f.values_of(G.MAP_IPV6, r.v6_keys), f.values_of(G.MAP_ETHERNET, r.eth_keys),
            f.values_of(G.MAP_PORTS, np.arange(65536, dtype=np.uint32))]


def test_all_selected_equals_classify_descs(G):
    """Verdicts pre-filled with PASS: the call is xfg_classify_descs over the
    batch on a fresh context."""
    rules, _, lens, umem, addr, ov = traffic()
    n = 4097
    rec = np.stack([addr[:n], lens[:n].astype(np.uint64)], axis=1)
    descs, first, mask = ring_around(rec, 8192 - 777)
    got = []
    for chained in (False, True):
        f = opened(G, DNY_ALL, rules)
        dev = Bufs(f)
        try:
            d_u, d_rx = dev(umem.nbytes, umem), dev(descs.nbytes, descs)
            d_v = dev(n, np.full(n, PASS, np.uint8))
            if chained:
                assert f.classify_descs_chain(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask) == (n, 0)
            else:
                f.classify_descs(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask)
            f.sync()
            got.append(results(G, f, rules, d_v, n) + [f.last_path()])
        finally:
            dev.free()
            f.close()
    for x, y in zip(*got):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(got[1][0], ov[:n])
    assert got[0][1].any() and got[0][2].any()


def test_fixed_stride_lengths_past_the_slot_are_clamped(G):
    """Some lens[i] > stride: the result is the unchained xfg_classify over the
    selected frames (a slot bounds its frame)."""
    rules, data, lens, _, _, _ = traffic()
    n = T() + 77
    big = lens[:n].copy()
    big[::7] = STRIDE + 1000
    big[-1] = 65000
    v_in = verdicts_in(n, "random")
    idx, want_counts = M.chain_model(v_in, 1 << PASS)
    assert np.count_nonzero(big[idx] > STRIDE) > 10 and idx[-1] != n - 1
    sel = np.ascontiguousarray(data[:n * STRIDE].reshape(n, STRIDE)[idx]).reshape(-1)
    f, g = opened(G, DNY_ALL, rules), opened(G, DNY_ALL, rules)
    dev = Bufs(f)
    try:
        d_d, d_l, d_v = dev(n * STRIDE, data[:n * STRIDE]), dev(4 * n, big), dev(n, v_in)
        assert f.classify_chain(d_d.ptr, d_l.ptr, n, STRIDE, d_v.ptr) == want_counts
        f.sync()
        d_sd, d_sl, d_sv = dev(sel.nbytes, sel), dev(4 * len(idx), big[idx]), dev(len(idx))
        g.classify(d_sd.ptr, d_sl.ptr, len(idx), STRIDE, d_sv.ptr)
        g.sync()
        rf, rg = results(G, f, rules, d_v, n), results(G, g, rules, d_sv, len(idx))
        np.testing.assert_array_equal(rf[0], M.merge(v_in, idx, rg[0]))
        for x, y in zip(rf[1:], rg[1:]):
            np.testing.assert_array_equal(x, y)
        # ... and the oracle's over the slot-long prefixes
        ov, orules, ost = oracle_stage(DNY_ALL, data, big, rules, idx)
        np.testing.assert_array_equal(rg[0], ov)
        check_all(G, f, rules, None, orules, ost)
    finally:
        dev.free()
        f.close()
        g.close()


def test_kernel_choice(G):
    """descs_min_packets = 1: the pipelined kernel; the default at this size:
    the general one; a fixed-stride batch too runs the descriptor kernels."""
    rules, data, lens, _, _, _ = traffic()
    n = T() + 1
    v_in = verdicts_in(n, "alternating")
    got = []
    for opts, path in ((dict(descs_min_packets=1), "PATH_PIPELINE"), ({}, "PATH_GENERAL")):
        f = opened(G, DNY_ALL, rules, **opts)
        dev = Bufs(f)
        try:
            d_d, d_l, d_v = dev(n * STRIDE, data[:n * STRIDE]), dev(4 * n, lens[:n]), dev(n, v_in)
            assert f.classify_chain(d_d.ptr, d_l.ptr, n, STRIDE, d_v.ptr) == ((n + 1) // 2, n // 2)
            f.sync()
            assert f.last_path() == getattr(G.Filter, path)
            got.append(results(G, f, rules, d_v, n))
        finally:
            dev.free()
            f.close()
    for x, y in zip(*got):
        np.testing.assert_array_equal(x, y)
    assert got[0][1].any()


@pytest.mark.parametrize("form", FORMS)
def test_nothing_selected_changes_nothing(G, form):
    """chain_mask == 0, and a mask no verdict byte is in: counts {0, n}, no
    launch of a classify kernel, no statistic, no counter, no byte of the
    verdicts or of idx."""
    rules = traffic()[0]
    n = T() + 1
    v_in = verdicts_in(n, "mixed")
    f = opened(G, DNY_ALL, rules)
    dev = Bufs(f)
    try:
        s = Source(dev, n, form)
        d_v, d_i = dev(n, v_in), dev(4 * n, np.full(n, 0xA5A5A5A5, np.uint32))
        for mask in (0, 1 << 5 | 1 << 30):
            assert s.chain(f, d_v.ptr, mask, d_i.ptr) == (0, n)
            assert s.chain(f, d_v.ptr, mask, None) == (0, n)
        f.sync()
        with pytest.raises(OSError) as e:                           # nothing was ever launched
            f.last_path()
        assert e.value.errno == errno.ENOENT
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), v_in)
        np.testing.assert_array_equal(d_i.download(np.zeros(n, np.uint32)), np.full(n, 0xA5A5A5A5, np.uint32))
        assert not f.stats().any()
        check_all(G, f, rules, None, rules.prepared(), np.zeros((5, 2), np.uint64))
    finally:
        dev.free()
        f.close()


def test_two_stages_then_egress_on_a_caller_stream(G):
    """A's classify, B's chained call and the egress on one stream of the
    caller's, no synchronisation by the test in between."""
    import torch
    from test_gpu_egress import slots
    data, lens, rules_a, rules_b = two_stage()
    n = len(lens)
    fa = X.VARIANT_FEATURES["xdpfilt_alw_udp"]
    va, _, _ = X.run_oracle(fa, data, lens, rules_a, stride=STRIDE)
    idx, want_counts = M.chain_model(va, 1 << PASS)
    vb, orules_b, ost_b = oracle_stage(DNY_ALL, data, lens, rules_b, idx)
    v = M.merge(va, idx, vb)
    umem, addr = umem_of(data, lens, STRIDE, seed=3)
    rec = np.stack([addr, lens.astype(np.uint64)], axis=1)
    descs, first, mask = ring_around(rec, 0xfffffff0)
    E = 8192
    assert E >= n
    tx_h, fill_h = np.full((E, 2), A5, np.uint64), np.full(E, A5, np.uint64)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    a, b = opened(G, fa, rules_a), opened(G, DNY_ALL, rules_b)
    dev = Bufs(a)
    try:
        d_u, d_rx, d_v = dev(umem.nbytes, umem), dev(descs.nbytes, descs), dev(n, np.full(n, 0xA5, np.uint8))
        d_tx, d_fill, d_c = dev(tx_h.nbytes, tx_h), dev(fill_h.nbytes, fill_h), dev(16)
        a.sync()
        b.sync()
        a.classify_descs(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask, stream=sp)
        counts = b.classify_descs_chain(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask, stream=sp)
        b.ring_egress(d_rx.ptr, n, d_v.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                      rx_first=first, rx_mask=mask, tx_first=E - 100, tx_mask=E - 1,
                      fill_first=0xfffffff0, fill_mask=E - 1, stream=sp)
        stream.synchronize()
        assert counts == want_counts
        ec = d_c.download(np.zeros(2, np.uint64)).tolist()
        got_tx, got_fill = d_tx.download(np.zeros_like(tx_h)), d_fill.download(np.zeros_like(fill_h))
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), v)
        check_all(G, b, rules_b, None, orules_b, ost_b)
    finally:
        dev.free()
        a.close()
        b.close()
    m = v == PASS
    assert 0 < m.sum() < n
    assert ec == [int(m.sum()), int(n - m.sum())]
    tx_h[slots(E - 100, ec[0], E - 1)] = rec[m]
    fill_h[slots(0xfffffff0, ec[1], E - 1)] = addr[~m] & ADDR48
    np.testing.assert_array_equal(got_tx, tx_h)
    np.testing.assert_array_equal(got_fill, fill_h)


def test_flat_array_of_many_sockets_chained(G):
    """xfg_classify_socks with a flat array (three sockets, one empty), then a
    second context over that array with every verdict selected."""
    from test_gpu_socks import Case
    rules, data, lens, umem, addr, ov = traffic()
    counts = (T() - 3, 0, 70)
    n = sum(counts)
    rules_a, _ = X.random_rules(5, n4=50, n6=20, ne=5, nports=10)
    a, b = opened(G, DNY_ALL, rules_a, descs_min_packets=1), opened(G, DNY_ALL, rules)
    c = Case(a, counts, "ring", batch=(addr[:n], lens[:n], np.zeros(n, np.uint32)))
    dev = Bufs(a)
    try:
        d_u, d_flat = dev(umem.nbytes, umem), dev(16 * n, np.full((n, 2), A5, np.uint64))
        a.classify_socks(d_u.ptr, c.table(G), c.d_v.ptr, flat_ptr=d_flat.ptr)
        a.sync()
        assert b.classify_descs_chain(d_u.ptr, d_flat.ptr, n, c.d_v.ptr, chain_mask=0xffffffff) == (n, 0)
        b.sync()
        _, orules, ost = X.run_oracle(DNY_ALL, data[:n * STRIDE], lens[:n], rules, stride=STRIDE)
        check_all(G, b, rules, ov[:n], orules, ost, c.d_v.download(np.zeros(n, np.uint8)))
    finally:
        dev.free()
        c.free()
        a.close()
        b.close()


def test_timed_call(G):
    rules, data, lens, umem, addr, ov = traffic()
    n = 3 * T() + 5
    v_in = verdicts_in(n, "random")
    idx, want_counts = M.chain_model(v_in, 1 << PASS)
    rec = np.stack([addr[:n], lens[:n].astype(np.uint64)], axis=1)
    got = []
    for timed in (False, True):
        f = opened(G, DNY_ALL, rules)
        dev = Bufs(f)
        try:
            d_u, d_rx, d_v = dev(umem.nbytes, umem), dev(rec.nbytes, rec), dev(n, v_in)
            if timed:
                counts, ms = f.classify_descs_chain_timed(d_u.ptr, d_rx.ptr, n, d_v.ptr)
                assert len(ms) == 3 and all(0 <= m < 1000 for m in ms)
                assert f.classify_descs_chain_timed(d_u.ptr, d_rx.ptr, n, d_v.ptr, chain_mask=0) == \
                    ((0, n), (0.0, 0.0, 0.0))
                c2, ms2 = f.classify_descs_chain_timed(d_u.ptr, d_rx.ptr, n, d_v.ptr, chain_mask=1 << 7)
                assert c2 == (0, n) and ms2[0] > 0 and ms2[1:] == (0.0, 0.0)
            else:
                counts = f.classify_descs_chain(d_u.ptr, d_rx.ptr, n, d_v.ptr)
            f.sync()
            assert counts == want_counts
            got.append(results(G, f, rules, d_v, n))
        finally:
            dev.free()
            f.close()
    for x, y in zip(*got):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(got[0][0], M.merge(v_in, idx, ov[:n][idx]))


@pytest.mark.parametrize("k", range(3), ids=["T-1", "T+1", "3T+7"])
def test_two_threads_share_the_frags_scratch(filt, k):
    """xfg_classify_descs_frags and xfg_classify_descs_chain size and use the
    same library scratch under one lock.  Two threads on one context and one
    device, 20 calls each over batches of different sizes, no pkt_of and no
    idx passed: every call gives the verdicts and counts the same call gave
    alone beforehand."""
    import threading
    from test_gpu_frags import NCHUNK, head_records, options_of
    sizes = [T() - 1, T() + 1, 3 * T() + 7]
    nf, nc = sizes[k], sizes[(k + 1) % 3]
    opts, v_in = options_of(nf, "random"), verdicts_in(nc, "random")
    dev = Bufs(filt)
    try:
        d_u = dev(NCHUNK * 64, np.zeros(NCHUNK * 64, np.uint8))
        d_rx, d_vf, d_vc = dev(16 * nf, head_records(opts)), dev(nf), dev(nc)
        s = Source(dev, nc, "ring", src=np.arange(nc) % NFRAMES)

        def frags():
            d_vf.upload(np.full(nf, 0xA5, np.uint8))
            counts = filt.classify_descs_frags(d_u.ptr, d_rx.ptr, nf, d_vf.ptr)
            return counts, d_vf.download(np.zeros(nf, np.uint8))

        def chain():
            d_vc.upload(v_in)
            counts = s.chain(filt, d_vc.ptr, 1 << PASS)
            return counts, d_vc.download(np.zeros(nc, np.uint8))

        alone = [frags(), chain()]
        assert alone[0][0][0] > 0 and alone[1][0][0] > 0
        got = [[], []]

        def worker(i, call):
            for _ in range(20):
                got[i].append(call())

        threads = [threading.Thread(target=worker, args=(i, call), daemon=True)
                   for i, call in enumerate((frags, chain))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=60)
        assert not any(t.is_alive() for t in threads), "a thread is still in its calls"
    finally:
        dev.free()
    for i in range(2):
        assert len(got[i]) == 20
        for counts, v in got[i]:
            assert counts == alone[i][0]
            np.testing.assert_array_equal(v, alone[i][1])

"""Multi-buffer AF_XDP packets of many sockets in one call
(xfg_classify_socks_frags, xfg_socks_frags_egress, xfg_socks_frags.hip).

Every case runs one poll round -- classify, then egress on the same stream with
no synchronisation between them beyond the classify's own -- and compares three
things: the verdict bytes (the whole array, XFG_VERDICT_NONE included), pkt_of,
done[] and the counts; every ring and every egress count; the rule values and
the statistics.  Each is compared twice: against the model (sockfragmodel.py,
checked on the CPU against hand-written rows and a plain walk) with the CPU
oracle's verdicts on the head frames, and against the per-socket loop of
xfg_classify_descs_frags and xfg_ring_egress(XFG_EGRESS_MULTIBUF) run on a
second context with the same rules.  Every comparison is exact; every output
ring is uploaded as 0xA5 bytes and compared whole.

The layouts are the smallest that reach the places the kernels can go wrong:
tiles of 2048 records and waves of 64, so about three tiles."""
import errno
import functools

import numpy as np
import pytest

import xftools as X
from sockfragmodel import PASS, classify_model, egress_model, spread, swapped
from sockmodel import bases
from test_gpu_descs import CHUNK, STRIDE, check_all, layout_const, umem_of
from test_gpu_egress import A5, ADDR48, records, slots
from test_gpu_socks import Case

pytestmark = pytest.mark.gpu

CONTD = 1
A5_32 = 0xA5A5A5A5


@functools.lru_cache(maxsize=None)
def T():
    return layout_const("XFG_SOCKS_TILE")


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


def random_cont(rng, n):
    """Packets of 1-4 records: 1 on every record but a packet's last."""
    ends = np.cumsum(rng.integers(1, 5, n + 1)) - 1
    c = np.ones(n, np.uint32)
    c[ends[ends < n]] = 0
    return c


# totals for the spread's lead, groups and tail: fewer records than a group, and next to tile edges
ODD = {"odd_1": lambda: 1, "odd_3": lambda: 3, "odd_5": lambda: 5, "odd_tile_less": lambda: T() - 1,
       "odd_tile_more": lambda: T() + 1, "odd_three_tiles": lambda: 3 * T() + 7}


@functools.lru_cache(maxsize=None)
def layout(name):
    """(records a socket, XDP_PKT_CONTD of every flat record), read only."""
    t = T()
    rng = np.random.default_rng(5 + len(name))
    if name == "edges":
        counts = [0, 0,              # empty sockets first
                  1, 2, 3, 57, 1,    # boundaries inside one wave; the last on the wave's edge
                  64,                # from a wave edge to the next
                  5,                 # continuation records only, between live sockets
                  t - 133,           # ends on the tile edge, its trailing packet with it
                  t + 100,           # its head opens the next tile; carried over two tiles
                  0, 0,              # a run of empty sockets
                  4,                 # one whole packet
                  1,
                  t - 98,            # to 3 tiles and 7 records
                  0, 0, 0]           # empty sockets last
        base = bases(counts)
        assert base[9] + counts[9] == t == base[10] and base[-1] == 3 * t + 7
        c = random_cont(rng, int(base[-1]))
        c[base[8]:base[9]] = 1
        c[t - 4], c[t - 3:t] = 0, 1                    # three trailing records up to the tile edge
        c[2 * t - 3], c[2 * t - 2:2 * t + 1], c[2 * t + 1] = 0, 1, 0    # a packet over the tile edge
        c[base[13]:base[14]] = [1, 1, 1, 0]
        c[base[14]] = 0
        c[-2:] = 1                                     # the last socket ends inside a packet
    elif name == "many":
        counts = [int(k) for k in np.random.default_rng(1024).integers(0, 4, 1024)]
        counts[0] = counts[1] = counts[-1] = 0
        c = (rng.random(sum(counts)) < 0.5).astype(np.uint32)
    elif name == "one":
        counts = [3 * t + 7]
        c = random_cont(rng, counts[0])
        c[-2:] = 1
    elif name in ("tile_less", "tile", "tile_more"):
        # one tile less a record, one tile, and one tile and a record: the first look-back
        counts = [t - 65, 64 + ("tile_less", "tile", "tile_more").index(name)]
        c = random_cont(rng, sum(counts))
        c[-2:] = 1
    elif name == "no_eop":
        counts = [1, 1, 2, 3, 57, 1, 63, 64, 65]
        c = np.ones(sum(counts), np.uint32)
    elif name in ODD:
        # two sockets; the first ends in up to five trailing records behind a whole packet
        total = ODD[name]()
        counts = [(total + 1) // 2, total // 2]
        c = random_cont(rng, total)
        c[-1] = 0
        k = min(counts[0] - 1, 5)
        if k:
            c[counts[0] - k - 1], c[counts[0] - k:counts[0]] = 0, 1
    c.setflags(write=False)
    return tuple(counts), c


@pytest.fixture(scope="module")
def traffic():
    """A few IPv4 and port rules under xdpfilt_dny_all and a fuzz frame for
    every record of the largest layout, each in a chunk of its own (read only);
    the oracle over the head frames of a layout, computed once."""
    rules, pool = X.random_rules(77, n4=8, n6=2, ne=2, nports=6)
    most = 3 * T() + 7
    data, lens = X.gen_fuzz(31, most, STRIDE, rules, pool)
    umem, addr = umem_of(data, lens, STRIDE, seed=9)
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    for a in (data, lens, umem, addr):
        a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def oracle(name):
        counts, cont = layout(name)
        heads = classify_model(counts, cont)[2]
        hd = data.reshape(-1, STRIDE)[:len(cont)][heads]
        return X.run_oracle(feats, np.ascontiguousarray(hd).reshape(-1), lens[:len(cont)][heads], rules,
                            stride=STRIDE)

    return rules, feats, data, lens, umem, addr, oracle


def check_rings(c, tx, fill, out, shared):
    """Counts and every ring whole (Case.check of test_gpu_socks.py with the
    model's results passed in)."""
    want_tx, want_fill, want_sfill = c.tx_h.copy(), c.fill_h.copy(), c.sfill_h.copy()
    for s in range(c.S):
        want_tx[c.off[s, 1] + c.at(s, 1, len(tx[s]))] = tx[s]
        if not shared:
            want_fill[c.off[s, 2] + c.at(s, 2, len(fill[s]))] = fill[s]
    if shared:
        want_sfill[slots(c.shared.first[2], len(fill), c.shared.mask[2])] = fill
    np.testing.assert_array_equal(c.d_c.download(np.zeros(2 * c.S + 2, np.uint64)), out)
    np.testing.assert_array_equal(c.d_tx.download(np.zeros_like(c.tx_h)), want_tx)
    np.testing.assert_array_equal(c.d_fill.download(np.zeros_like(c.fill_h)), want_fill)
    np.testing.assert_array_equal(c.d_sfill.download(np.zeros_like(c.sfill_h)), want_sfill)


def per_socket_loop(G, g, cg, d_u, d_p, shared, flags, all_live):
    """The round with the existing calls: xfg_classify_descs_frags and
    xfg_ring_egress(MULTIBUF) a socket, the shared fill ring's index carried
    from socket to socket.  Returns done[] and the packets a socket."""
    done, npk = np.zeros(cg.S, np.uint32), np.zeros(cg.S, np.int64)
    fill_at = cg.shared.first[2]
    for s, r in enumerate(cg.rings):
        cnt, b = int(cg.counts[s]), int(cg.base[s])
        rx = cg.d_rx.ptr + 16 * int(cg.off[s, 0])
        k = g.classify_descs_frags(d_u.ptr, rx, cnt, cg.d_v.ptr + b, pkt_of_ptr=d_p.ptr + 4 * b,
                                   first=r.first[0], mask=r.mask[0])
        npk[s], done[s] = k[0], k[1]
        own = cg.d_fill.ptr + 8 * int(cg.off[s, 2]) if cg.has_fill[s] else None
        g.ring_egress(rx, cnt if all_live else k[1], cg.d_v.ptr + b, cg.d_c.ptr + 16 * s,
                      tx_ptr=cg.d_tx.ptr + 16 * int(cg.off[s, 1]) if cg.has_tx[s] else None,
                      fill_ptr=cg.d_sfill.ptr if shared else own,
                      rx_first=r.first[0], rx_mask=r.mask[0], tx_first=r.first[1], tx_mask=r.mask[1],
                      fill_first=fill_at if shared else r.first[2],
                      fill_mask=cg.shared.mask[2] if shared else r.mask[2],
                      umem_ptr=d_u.ptr, flags=flags | G.EGRESS_MULTIBUF)
        if shared:
            g.sync()
            got = cg.d_c.download(np.zeros(2 * cg.S + 2, np.uint64))
            fill_at = (fill_at + int(got[2 * s + 1])) & 0xffffffff
    g.sync()
    return done, npk


def run_round(G, traffic, name, kind, shared, no_tx=(), no_fill=(), swap=False, flat=True,
              stream=False, all_live=False, min_packets=None, v_off=0):
    import torch
    rules, feats, data, lens, umem, addr, oracle = traffic
    counts, cont = layout(name)
    n, S = len(cont), len(counts)
    assert not set(no_tx) & set(no_fill)
    opts = cont | np.where(np.arange(n) % 5 == 4, 1 << 16, 0).astype(np.uint32)
    batch = (addr[:n], lens[:n], opts)
    done, pkt_of, heads, c3 = classify_model(counts, opts)
    if c3[0]:
        ov, orules, ost = oracle(name)
        assert n < 64 or 0 < np.count_nonzero(ov == PASS) < c3[0]
    else:
        ov, orules, ost = np.zeros(0, np.uint8), rules.prepared(), np.zeros((5, 2), np.uint64)
    want_v = spread(pkt_of, ov)
    kw = {} if min_packets is None else dict(descs_min_packets=min_packets)
    flags = G.EGRESS_SWAP_MACS if swap else 0
    f, g = G.Filter(feats, ndev=1, **kw), G.Filter(feats, ndev=1, **kw)
    f.load_rules(rules)
    g.load_rules(rules)
    c = Case(f, counts, kind, batch=batch, no_tx=no_tx, no_fill=no_fill)
    cg = Case(g, counts, kind, batch=batch, no_tx=no_tx, no_fill=no_fill)
    extra = [f.alloc(umem.nbytes), g.alloc(umem.nbytes), f.alloc(4 * n + 4), g.alloc(4 * n + 4),
             f.alloc(16 * n), f.alloc(n + 16)]
    d_u, d_ug, d_p, d_pg, d_flat, d_vo = extra
    # (v_off: the verdict bytes at that offset of an allocation of their own, 0xA5 around them)
    v_ptr = d_vo.ptr + v_off if v_off else c.d_v.ptr
    try:
        for d in (d_u, d_ug):
            d.upload(umem)
        for d in (d_p, d_pg):
            d.upload(np.full(n + 1, A5_32, np.uint32))
        d_flat.upload(np.full((n, 2), A5, np.uint64))
        d_vo.upload(np.full(n + 16, 0xA5, np.uint8))
        for k in (c, cg):
            k.d_v.upload(np.full(max(n, 16), 0xA5, np.uint8))
            k.reset_outputs()
        f.sync()
        st = torch.cuda.Stream() if stream else None
        sp = st.cuda_stream if st else None
        # the round: one classify, one egress, nothing between them
        got_done, got_c3 = f.classify_socks_frags(d_u.ptr, c.table(G), v_ptr, pkt_of_ptr=d_p.ptr,
                                                  flat_ptr=d_flat.ptr if flat else None, stream=sp)
        f.socks_frags_egress(c.table(G), v_ptr, c.d_c.ptr, done=None if all_live else got_done,
                             fill_ptr=c.d_sfill.ptr if shared else None,
                             fill_first=c.shared.first[2], fill_mask=c.shared.mask[2],
                             umem_ptr=d_u.ptr, flags=flags, stream=sp)
        if st:
            st.synchronize()
        f.sync()
        # 1: against the model and the oracle
        np.testing.assert_array_equal(got_done, done)
        assert got_c3 == c3 and c3[1] + c3[2] == n
        v = c.d_v.download(np.zeros(max(n, 16), np.uint8))[:n]
        if v_off:
            assert np.all(v == 0xA5)
            around = d_vo.download(np.zeros(n + 16, np.uint8))
            v = around[v_off:v_off + n]
            assert np.all(around[:v_off] == 0xA5) and np.all(around[v_off + n:] == 0xA5)
        np.testing.assert_array_equal(v, want_v)
        p = d_p.download(np.zeros(n + 1, np.uint32))
        np.testing.assert_array_equal(p[:n], pkt_of)
        assert p[n] == A5_32
        np.testing.assert_array_equal(d_flat.download(np.zeros((n, 2), np.uint64)),
                                      records(*batch) if flat else np.full((n, 2), A5, np.uint64))
        live_done = None if all_live else done
        tx, fill, out = egress_model(counts, live_done, batch[0], batch[1], opts, want_v, c.has_tx,
                                     c.has_fill, shared)
        check_rings(c, tx, fill, out, shared)
        assert int(out[2 * S]) + int(out[2 * S + 1]) == (n if all_live else c3[1])
        if c3[0]:
            assert f.last_path() == (G.Filter.PATH_PIPELINE if min_packets == 1 else
                                     G.Filter.PATH_GENERAL)
        check_all(G, f, rules, None, orules, ost)
        want_u = umem.copy()
        if swap:      # head frames swapped, continuation chunks byte-identical
            sel = swapped(counts, live_done, opts, want_v, c.has_tx)
            assert 0 < sel.sum() < np.count_nonzero(want_v == PASS)
            start = ((batch[0] & ADDR48) + (batch[0] >> np.uint64(48))).astype(np.int64)
            at = start[sel][:, None] + np.arange(12)
            want_u[at] = umem[at][:, [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]]
        got_u = d_u.download(np.zeros_like(umem))
        np.testing.assert_array_equal(got_u, want_u)
        # 2: against the per-socket loop of the existing calls on a second context
        loop_done, loop_npk = per_socket_loop(G, g, cg, d_ug, d_pg, shared, flags, all_live)
        np.testing.assert_array_equal(loop_done, got_done)
        assert int(loop_npk.sum()) == got_c3[0]
        sock = np.repeat(np.arange(S), counts)
        live = (np.arange(n) - cg.base[sock]) < loop_done[sock].astype(np.int64)
        vg = cg.d_v.download(np.zeros(max(n, 16), np.uint8))[:n]
        np.testing.assert_array_equal(vg[live], v[live])
        assert np.all(vg[~live] == 0xA5) and np.all(v[~live] == G.VERDICT_NONE)
        pg = d_pg.download(np.zeros(n + 1, np.uint32))[:n]
        first_pkt = np.cumsum(loop_npk) - loop_npk       # a socket's first flat packet index
        np.testing.assert_array_equal((pg + first_pkt[sock].astype(np.uint32))[live], p[:n][live])
        assert np.all(p[:n][~live] == G.PKT_NONE)
        for a, b in ((c.d_tx, cg.d_tx), (c.d_fill, cg.d_fill), (c.d_sfill, cg.d_sfill)):
            np.testing.assert_array_equal(a.download(np.zeros(a.nbytes, np.uint8)),
                                          b.download(np.zeros(b.nbytes, np.uint8)))
        cf = c.d_c.download(np.zeros(2 * S + 2, np.uint64))
        cl = cg.d_c.download(np.zeros(2 * S + 2, np.uint64))
        np.testing.assert_array_equal(cf[:2 * S], cl[:2 * S])
        assert [int(cf[2 * S]), int(cf[2 * S + 1])] == [int(cl[0:2 * S:2].sum()), int(cl[1:2 * S:2].sum())]
        np.testing.assert_array_equal(g.stats(), f.stats())
        r = rules.prepared()
        for m, keys in ((G.MAP_IPV4, r.v4_keys), (G.MAP_IPV6, r.v6_keys), (G.MAP_ETHERNET, r.eth_keys),
                        (G.MAP_PORTS, np.arange(65536, dtype=np.uint32))):
            np.testing.assert_array_equal(g.values_of(m, keys), f.values_of(m, keys))
        np.testing.assert_array_equal(d_ug.download(np.zeros_like(umem)), got_u)
        return got_c3, out
    finally:
        for b in extra:
            b.free()
        c.free()
        cg.free()
        f.close()
        g.close()


ROUNDS = {
    # rings that wrap (a first at 0xfffffff0 on every socket), per-socket fill, a flat array, a
    # caller's stream
    "edges_ring_own_stream": dict(name="edges", kind="ring", shared=False, stream=True),
    # the shared fill ring, no flat array, the library's stream, sockets without a TX ring, the swap
    "edges_ring_shared_swap": dict(name="edges", kind="ring", shared=True, flat=False, swap=True,
                                   no_tx=(3, 10)),
    # plain arrays, sockets without a TX ring or without a fill ring, the heads on the pipelined kernel
    "edges_array_own_pipelined": dict(name="edges", kind="array", shared=False, no_tx=(5, 9),
                                      no_fill=(7, 10, 15), min_packets=1, swap=True),
    # done == NULL: every record live, the trailing ones on the fill side
    "edges_ring_shared_all_live": dict(name="edges", kind="ring", shared=True, all_live=True,
                                       stream=True),
    "edges_array_own_all_live": dict(name="edges", kind="array", shared=False, all_live=True,
                                     flat=False, swap=True),
    # the largest table, 0-3 records a socket
    "many_ring_own": dict(name="many", kind="ring", shared=False, flat=False),
    "many_array_shared_swap": dict(name="many", kind="array", shared=True, swap=True, stream=True,
                                   no_tx=(5, 6, 7, 500)),
    # batches that end next to the first tile's edge
    "tile_less_ring_own": dict(name="tile_less", kind="ring", shared=False),
    "tile_array_shared": dict(name="tile", kind="array", shared=True, flat=False),
    "tile_more_ring_shared": dict(name="tile_more", kind="ring", shared=True, stream=True),
    # one socket alone: xfg_classify_descs_frags and xfg_ring_egress themselves
    "one_ring_own": dict(name="one", kind="ring", shared=False),
    "one_ring_shared": dict(name="one", kind="ring", shared=True, flat=False, swap=True),
}


@pytest.mark.parametrize("case", list(ROUNDS))
def test_round(G, traffic, case):
    c3, out = run_round(G, traffic, **ROUNDS[case])
    assert c3[0] > 0 and c3[2] > 0               # packets, and trailing records somewhere


@pytest.mark.parametrize("name", list(ODD))
@pytest.mark.parametrize("v_off", [1, 2, 3])
def test_round_with_the_verdicts_off_a_4_byte_boundary(G, traffic, name, v_off):
    """The spread's lead bytes, whole groups and tail over all records,
    XFG_VERDICT_NONE on the trailing ones, and nothing written around them."""
    c3, out = run_round(G, traffic, name=name, kind="ring", shared=False, v_off=v_off)
    n = ODD[name]()
    assert c3[0] > 0 and c3[2] == min((n + 1) // 2 - 1, 5) and c3[1] + c3[2] == n


@pytest.mark.parametrize("shared", [False, True], ids=["own_fill", "shared_fill"])
def test_no_end_of_packet_at_all(G, traffic, shared):
    """{0, 0, total}, every verdict XFG_VERDICT_NONE, no statistic changes, no
    ring entry; with done == NULL every chunk goes back."""
    c3, out = run_round(G, traffic, name="no_eop", kind="ring", shared=shared)
    n = len(layout("no_eop")[1])
    assert c3 == (0, 0, n) and not out.any()
    c3, out = run_round(G, traffic, name="no_eop", kind="ring", shared=shared, all_live=True)
    assert c3 == (0, 0, n) and int(out[-1]) == n and int(out[-2]) == 0


def test_an_empty_round_and_the_refused_flag(G, traffic):
    rules, feats = traffic[0], traffic[1]
    f = G.Filter(feats, ndev=1)
    f.load_rules(rules)
    c = Case(f, [0, 0, 0], "array")
    try:
        before = f.stats()
        c.reset_outputs()
        done, c3 = f.classify_socks_frags(None, c.table(G), None)
        assert done.tolist() == [0, 0, 0] and c3 == (0, 0, 0)
        for shared in (False, True):
            f.socks_frags_egress(c.table(G), None, c.d_c.ptr, done=done,
                                 fill_ptr=c.d_sfill.ptr if shared else None)
        f.sync()
        check_rings(c, [np.zeros((0, 2), np.uint64)] * 3, [np.zeros(0, np.uint64)] * 3,
                    np.zeros(8, np.uint64), False)
        np.testing.assert_array_equal(f.stats(), before)
        # xfg_socks_egress still refuses XFG_EGRESS_MULTIBUF
        tab = G.sock_table([dict(rx_descs=c.d_rx.ptr, tx_descs=c.d_tx.ptr, fill_addrs=c.d_fill.ptr,
                                 count=1)])
        for flags in (G.EGRESS_MULTIBUF, G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS):
            with pytest.raises(OSError) as e:
                f.socks_egress(tab, c.d_v.ptr, c.d_c.ptr, umem_ptr=c.d_rx.ptr, flags=flags)
            assert e.value.errno == errno.EINVAL
        # done[s] above the socket's count
        with pytest.raises(OSError) as e:
            f.socks_frags_egress(tab, c.d_v.ptr, c.d_c.ptr, done=[2])
        assert e.value.errno == errno.EINVAL
    finally:
        c.free()
        f.close()

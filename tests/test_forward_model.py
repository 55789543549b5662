"""tests/fwdmodel.py against xdp-forward's program text, branch by branch
(xdp-forward/xdp_forward.bpf.c:23-127, headers/xdp/parsing_helpers.h:100-134
and :201-233), and the conditions the GPU corpus (tests/fwdcorpus.py) has to
meet, asserted on the model alone."""
import numpy as np
import pytest

import fwdcorpus as K
import fwdmodel as M

Q, AD = M.ETH_P_8021Q, M.ETH_P_8021AD
DST = M.ip_bytes(0x0a010203)
NEXTHOPS = [(5, 0, 0, b"\x02\x01\x00\x00\x00\x05", b"\x02\x02\x00\x00\x00\x05"),
            (6, 0, 4, b"\x02\x01\x00\x00\x00\x06", b"\x02\x02\x00\x00\x00\x06"),      # ret != 0
            (7, 100, 0, b"\x02\x01\x00\x00\x00\x07", b"\x02\x02\x00\x00\x00\x07"),    # mtu 100
            (8, 0, 0, b"\x02\x01\x00\x00\x00\x08", b"\x02\x02\x00\x00\x00\x08")]      # not a port
ROUTES = [(0x0a000000, 8, 0), (0x0b000000, 8, 1), (0x0c000000, 8, 2), (0x0d000000, 8, 3)]
PORTS = [7, 5]


def fwd(f):
    return M.forward_frame(f, lambda d: M.lpm(ROUTES, d), NEXTHOPS, PORTS)


def v4(dst=DST, tags=(), **kw):
    return M.eth(M.ETH_P_IP, M.ipv4(dst, **kw), tags)


def test_every_reason_by_hand():
    rows = [(v4(), M.OK, 1),
            (b"\x00" * 13, M.NOT_IP, None),
            (M.eth(M.ETH_P_ARP, bytes(28)), M.NOT_IP, None),
            (v4()[:33], M.BAD_HDR, None),
            (v4(ttl=1), M.TTL, None),
            (v4(ttl=0), M.TTL, None),
            (M.eth(M.ETH_P_IPV6, bytes(40)), M.V6, None),
            (M.eth(M.ETH_P_IPV6, b""), M.V6, None),           # not parsed further
            (v4(M.ip_bytes(0x0e000001)), M.NO_ROUTE, None),
            (v4(M.ip_bytes(0x0b000001)), M.NH_RET, None),
            (v4(M.ip_bytes(0x0c000001), tot_len=101), M.FRAG, None),
            (v4(M.ip_bytes(0x0c000001), tot_len=100), M.OK, 0),
            (v4(M.ip_bytes(0x0c000001), payload=bytes(76), tot_len=20), M.OK, 0),   # the field, not len
            (v4(M.ip_bytes(0x0d000001)), M.NO_PORT, None)]
    assert {r for _, r, _ in rows} == set(range(M.REASONS))
    for f, reason, q in rows:
        got = fwd(f)
        assert got[:2] == (reason, q), (f.hex(), M.REASON_NAMES[reason])
        if reason != M.OK:
            assert got[2] == f


def test_the_order_of_the_rows():
    """TTL before the lookup's reasons; NH_RET before FRAG before NO_PORT."""
    assert fwd(v4(M.ip_bytes(0x0e000001), ttl=1))[0] == M.TTL
    nh = list(NEXTHOPS)
    nh[1] = (99, 100, 4, b"\0" * 6, b"\0" * 6)          # ret, small mtu and no port at once
    f = v4(M.ip_bytes(0x0b000001), tot_len=500)
    assert M.forward_frame(f, lambda d: M.lpm(ROUTES, d), nh, PORTS)[0] == M.NH_RET
    nh[1] = (99, 100, 0, b"\0" * 6, b"\0" * 6)
    assert M.forward_frame(f, lambda d: M.lpm(ROUTES, d), nh, PORTS)[0] == M.FRAG


@pytest.mark.parametrize("ntags", range(6))
def test_tag_counts(ntags):
    tags = tuple([AD, Q][k % 2] for k in range(ntags))
    f = v4(tags=tags)
    r, q, g = fwd(f)
    if ntags <= 4:
        l3 = 14 + 4 * ntags
        assert (r, q) == (M.OK, 1)
        assert g[12:l3] == f[12:l3]                      # the tags stay
        assert g[l3 + 8] == f[l3 + 8] - 1
    else:
        assert r == M.NOT_IP and g == f                  # a fifth tag leaves a VLAN ethertype


@pytest.mark.parametrize("ntags", [1, 2, 3, 4])
def test_a_tag_cut_at_every_length(ntags):
    """The frame ends 0..3 bytes into its last tag: the loop ends with the VLAN
    ethertype (:123-124); with the whole tag there and nothing behind, an IPv4
    header that does not fit."""
    f = v4(tags=(Q,) * ntags)
    for cut in range(4):
        assert fwd(f[:14 + 4 * (ntags - 1) + cut])[0] == M.NOT_IP
    assert fwd(f[:14 + 4 * ntags])[0] == M.BAD_HDR


@pytest.mark.parametrize("ihl", range(16))
def test_ihl_against_len(ihl):
    """l3 + 20 and l3 + 4 * ihl must both fit; no ihl >= 5 check."""
    f = v4(ihl=ihl, payload=bytes(8))
    hdr = 14 + 4 * max(ihl, 5)
    assert fwd(f[:hdr])[0] == M.OK
    assert fwd(f[:14 + max(20, 4 * ihl) - 1])[0] == M.BAD_HDR
    if ihl < 5:
        assert fwd(f[:14 + 20])[0] == M.OK and fwd(f[:14 + 19])[0] == M.BAD_HDR


@pytest.mark.parametrize("ttl,reason", [(0, M.TTL), (1, M.TTL), (2, M.OK), (255, M.OK)])
def test_ttl(ttl, reason):
    r, _, g = fwd(v4(ttl=ttl))
    assert r == reason
    if reason == M.OK:
        assert g[14 + 8] == ttl - 1


@pytest.mark.parametrize("stored,after", [(0xFFFE, 0x0000), (0xFFFF, 0x0001), (0xFEFF, 0xFF00),
                                          (0x0000, 0x0001)])
def test_the_checksum_step_is_literal(stored, after):
    """:25-28 on the value a little-endian 16-bit load of the field gives:
    check += htons(0x0100) (1, so loaded); + 1 if that is >= 0xFFFF; truncated."""
    c = stored + 0x0001
    assert M.decrease_ttl(stored) == after == (c + (c >= 0xFFFF)) & 0xffff
    f = bytearray(v4())
    f[24:26] = stored.to_bytes(2, "little")
    g = fwd(bytes(f))[2]
    assert int.from_bytes(g[24:26], "little") == after


def test_random_valid_headers_stay_valid():
    rng = np.random.default_rng(1)
    for k in range(10000):
        b = lambda m: bytes(rng.integers(0, 256, m, dtype=np.uint8))     # noqa: E731
        ihl = int(rng.integers(5, 16))
        h = bytearray(M.ipv4(M.ip_bytes(0x0a000000 | int(rng.integers(1 << 24))), b(4),
                             int(rng.integers(2, 256)), int(rng.integers(256)), ihl=ihl,
                             tos=int(rng.integers(256)), ident=int(rng.integers(65536))))
        h[20:4 * ihl] = b(4 * ihl - 20)
        h[10:12] = bytes(2)
        h[10:12] = (~M.csum16(bytes(h)) & 0xffff).to_bytes(2, "big")
        assert M.csum16(bytes(h)) == 0xFFFF
        tags = (Q,) * (k % 5)
        r, _, g = fwd(M.eth(M.ETH_P_IP, bytes(h), tags))
        assert r == M.OK
        l3 = 14 + 4 * len(tags)
        assert M.csum16(g[l3:l3 + 4 * ihl]) == 0xFFFF


def test_lpm_many_is_lpm():
    routes, _ = K.fib_of(63)
    rng = np.random.default_rng(3)
    dsts = np.concatenate([rng.integers(0, 1 << 32, 3000, dtype=np.uint64),
                           np.array([K.inside(rng, routes[int(rng.integers(len(routes)))])
                                     for _ in range(3000)], np.uint64)])
    want = [M.lpm(routes, int(d)) for d in dsts]
    got = M.lpm_many(routes, dsts)
    assert [None if g < 0 else int(g) for g in got] == want


# ---- the GPU corpus's conditions
@pytest.mark.parametrize("nports", [1, 8, 63])
def test_corpus_conditions(nports):
    """As the GPU tests draw it: 3 * 2048 + 5 records, about 70% PASS."""
    routes, nexthops = K.fib_of(nports)
    pool = K.pool_of(nports)
    n = K.N3
    fid = np.random.default_rng(100 + n + nports).permutation(len(pool))[:n]
    v = K.verdicts_of(n, "random")
    lens = np.array([len(pool[k]) for k in fid])
    tx, fill, counts, qof, rof, after = M.forward_model(pool, fid, np.arange(n, dtype=np.uint64) * 128,
                                                        lens, v, routes, nexthops, K.ifindexes(nports))
    assert (counts[nports + 2:] >= 50).all(), counts[nports + 2:]
    assert (counts[:nports + 2] > 0).all()
    longest = {}
    for i in np.flatnonzero(rof == M.OK):
        f = pool[fid[i]]
        l3 = M.parse_ethhdr(f)[1]
        dst = int.from_bytes(f[l3 + 16:l3 + 20], "big")
        longest[i] = max(l for p, l, _ in routes if (dst & M.mask_of(l)) == p)
    deep = sum(1 for l in longest.values() if l > 24)
    # a /24 with a longer prefix in it resolves through its group whatever matches
    assert deep >= 50 and len(longest) - deep >= 50


def test_one_flow_corpus_takes_one_port_through_a_group():
    routes, nexthops = K.fib_of(8)
    pool = K.one_flow_pool()
    assert len(set(pool)) == len(pool)
    r, q, _ = M.forward_frame(pool[0], lambda d: M.lpm(routes, d), nexthops, K.ifindexes(8))
    assert r == M.OK and M.lpm(routes, 0x0a010281) == 3

"""Frames, FIBs and port tables for the tests of forwarded egress against the
reference's own xdp-forward program (oracle/ref/ref_forward_harness.c,
DESIGN.md §2).

Seeded and deterministic, built without a GPU.  One pool of distinct frames of
at most MAXLEN bytes, a chunk of its own each, so no frame is rewritten twice;
one route list, and a next-hop list and a port table for each of TABLES: 1, 8
and 63 ports (fwdcorpus.ifindexes) and "collide", 63 ports whose ifindexes all
hash to slots 126 and 127 of the kernel's 128-slot port hash, so the probe
chain runs through slot 0 to slot 60.  Every table's next hops end with two on
absent ifindexes; in "collide" the first hashes to slot 126 and walks the whole
chain to the empty slot 61, the second hashes to a slot nobody took.

Parts (PARTS; corpus().part):
  base    fwdcorpus.frame()'s sixteen kinds over this module's routes
  v6      IPv6 under 0-4 tags: the header cut at every length, hop_limit 0 / 1,
          whole headers; a chain of seven extension headers (cut at MAXLEN,
          which holds all the six-round loop of skip_ip6hdrext reads: it gives
          up); a fragment header
  check   routed IPv4 with stored check 0xFFFE, 0xFFFF, 0x0000, 0xFEFF (as the
          little-endian load sees them) x five tag depths x TTL 2 and 255
  ihl     ihl 0-15 at tag depths 0 and 4, cut at l3 + max(20, 4 * ihl) and one
          byte short of it
  short   IPv4 and IPv6 under 0-2 tags cut at 14, 17, 18, 33 and 34 bytes
  absent  frames for the second absent ifindex

Tags (TAGS; corpus().tag): the return statement of xdp_fwd_flags() the frame
reaches, known from how it was built (":N" are lines of
xdp-forward/xdp_forward.bpf.c), ":126" split by the lookup's answer:
  :49     parse_iphdr refused the header
  :52     ttl <= 1
  :68     parse_ip6hdr refused the header or its extension chain (a whole
          header with less than two bytes behind it among them)
  :71     hop_limit <= 1
  :82     neither IPv4 nor IPv6 (a frame below 14 bytes among them: parse_ethhdr
          returns -1)
  :114    the lookup succeeded, the ifindex is no port
  :123    redirected
  :126/1  no route     :126/2  a hop's ret     :126/3  FRAG_NEEDED
  :126/6  the lookup was called with AF_INET6
  lookup  an IPv4 frame that reaches the lookup with an address inside a
          random route: :114, :123 or :126 by the longest match
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import fwdcorpus as K
import fwdmodel as M

MAXLEN = 96
TILE = K.TILE
SEED = 7100
NBASE = 4 * TILE
TABLES = (1, 8, 63, "collide")
NGOOD = 126                         # good next hops in every table: two a port of the largest
PARTS = ["base", "v6", "check", "ihl", "short", "absent"]
TAGS = [":49", ":52", ":68", ":71", ":82", ":114", ":123", ":126/1", ":126/2", ":126/3", ":126/6", "lookup"]
# tag -> the stages (xftools.FWD_ST_*) the reference may report for it
STAGES_OF = {":49": {0}, ":52": {0}, ":68": {0}, ":71": {0}, ":82": {0}, ":114": {4}, ":123": {5},
             ":126/1": {1}, ":126/2": {2}, ":126/3": {3}, ":126/6": {6}, "lookup": {1, 2, 3, 4, 5}}
# tag -> fwdmodel's reason ("lookup": by the stage)
REASON_OF = {":49": M.BAD_HDR, ":52": M.TTL, ":68": M.V6, ":71": M.V6, ":82": M.NOT_IP, ":114": M.NO_PORT,
             ":123": M.OK, ":126/1": M.NO_ROUTE, ":126/2": M.NH_RET, ":126/3": M.FRAG, ":126/6": M.V6}
REASON_OF_STAGE = {1: M.NO_ROUTE, 2: M.NH_RET, 3: M.FRAG, 4: M.NO_PORT, 5: M.OK}
LE_CHECKS = (0xFFFE, 0xFFFF, 0x0000, 0xFEFF)
# destinations behind the fixed routes, by what the lookup answers
DST_OK = (0x0a010203, 0x0a0102c8, 0x0a010281, 0x0a017777, 0x0a555555)
NET_RET, NET_FRAG, NET_ABSENT_A, NET_ABSENT_B, NET_NONE = 0xc0a80000, 0xac100000, 0x0a090000, 0x0a0a0000, 0x0b000000


def fwd_hash(ifindex):
    """xfg_fwd_hash() of xdp-tools_amd/csrc/xfg_layout.h, restated to find
    ifindexes that collide: a coverage aid, no expected value depends on it."""
    return ((ifindex * 0x9e3779b1) & 0xffffffff) >> 25


def probe_distances(ifx):
    """How far from its home slot each port of ifx sits when the table is built
    in port order with linear probing (as the host builds it)."""
    taken, out = set(), []
    for i in ifx:
        d = 0
        while (fwd_hash(i) + d) % 128 in taken:
            d += 1
        taken.add((fwd_hash(i) + d) % 128)
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def colliding():
    """(ports, absent_a, absent_b): 63 ifindexes in slots 126 and 127, by turns;
    an absent one in slot 126; an absent one in slot 100, which stays empty."""
    by_slot = {126: [], 127: [], 100: []}
    i = 1
    while len(by_slot[126]) < 33 or len(by_slot[127]) < 32 or not by_slot[100]:
        if fwd_hash(i) in by_slot:
            by_slot[fwd_hash(i)].append(i)
        i += 1
    ports = [by_slot[126 + q % 2][q // 2] for q in range(63)]
    return ports, by_slot[126][32], by_slot[100][0]


def ifindexes(table):
    return colliding()[0] if table == "collide" else K.ifindexes(table)


def absent(table):
    return colliding()[1:] if table == "collide" else (K.IF_ABSENT, K.IF_ABSENT - 1)


@functools.lru_cache(maxsize=None)
def routes():
    """(prefix, len, nexthop) triples, the same for every table: fwdcorpus's
    fixed nested routes over 10.1.2.200 and its special routes, one more to the
    second absent ifindex, and random routes of lengths 8..32 inside 20.0.0.0/8
    to the good next hops by turns.  No default route; 11.0.0.0/8 has none."""
    rng = np.random.default_rng(SEED)
    out = {(0x0a000000, 8): 0, (0x0a010000, 16): 1, (0x0a010200, 24): 2, (0x0a010280, 25): 3,
           (0x0a0102c8, 32): 4, (NET_RET, 16): NGOOD, (NET_FRAG, 12): NGOOD + 1,
           (NET_ABSENT_A, 16): NGOOD + 2, (NET_ABSENT_B, 16): NGOOD + 3}
    for j in range(4 * 63 + 60):
        length = int(rng.integers(8, 33))
        prefix = (0x14000000 | int(rng.integers(1 << 24))) & M.mask_of(length)
        out.setdefault((prefix, length), 5 + j % (NGOOD - 5))
    return tuple((p, l, nh) for (p, l), nh in out.items())


@functools.lru_cache(maxsize=None)
def nexthops(table):
    """(ifindex, mtu, ret, dmac, smac) tuples: NGOOD good ones over the table's
    ports by turns (every third with mtu 1500), then a blackhole, one with mtu
    100 on the last port, and the two absent ifindexes."""
    ifx = ifindexes(table)
    a, b = absent(table)
    nh = [(ifx[k % len(ifx)], 0 if k % 3 else 1500, 0, K.mac(k, 1), K.mac(k, 2)) for k in range(NGOOD)]
    nh += [(ifx[0], 0, 3, K.mac(900, 1), K.mac(900, 2)),
           (ifx[-1], 100, 0, K.mac(901, 1), K.mac(901, 2)),
           (a, 0, 0, K.mac(902, 1), K.mac(902, 2)),
           (b, 0, 0, K.mac(903, 1), K.mac(903, 2))]
    return tuple(nh)


def sem(ntags, fam, n, ihl=5, ttl=64, then=":123"):
    """The tag of the first @n bytes of a frame built as Ethernet, @ntags <= 4
    VLAN tags and an IPv4 header claiming @ihl (fam 4) or a plain IPv6 header
    (fam 6) with @ttl as TTL / hop_limit; @then: what the lookup leads to."""
    if n < 14:
        return ":82"
    for j in range(ntags):
        if n < 18 + 4 * j:          # cut inside tag j: a VLAN ethertype is left
            return ":82"
    l3 = 14 + 4 * ntags
    if fam == 4:
        if n < l3 + 20 or n < l3 + 4 * ihl:
            return ":49"
        return ":52" if ttl <= 1 else then
    # (skip_ip6hdrext wants two bytes behind the header whatever nexthdr is:
    # parsing_helpers.h:144 stands in front of the switch)
    if n < l3 + 42:
        return ":68"
    return ":71" if ttl <= 1 else ":126/6"


class Corpus(NamedTuple):
    frames: tuple           # the frames' bytes, distinct chunks
    lens: np.ndarray        # u32
    part: np.ndarray        # u8 index into PARTS
    tag: np.ndarray         # u8 index into TAGS


BASE_TAG = {9: ":126/1", 10: ":52", 11: ":126/6", 12: ":49", 13: ":82", 14: ":82", 15: ":82"}
SPECIAL_TAG = [":126/2", ":126/3", ":123", ":114"]      # fwdcorpus.frame()'s kind 8, by turns


def ipv6(nexthdr, hop_limit, rest, r):
    return bytes([0x60, 0, 0, 0]) + len(rest).to_bytes(2, "big") + bytes([nexthdr, hop_limit]) + r(32) + rest


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    """Built once; do not modify."""
    rng = np.random.default_rng(SEED + 1)
    r = lambda m: bytes(rng.integers(0, 256, m, dtype=np.uint8))     # noqa: E731
    rt = routes()
    frames, part, tag = [], [], []

    def add(p, f, t):
        assert len(f) <= MAXLEN, (p, len(f))
        frames.append(bytes(f))
        part.append(PARTS.index(p))
        tag.append(TAGS.index(t))

    def v4(dst, tags=(), **kw):
        kw.setdefault("ident", len(frames) & 0xffff)
        return M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(dst), r(4), **kw), tags)

    for k in range(NBASE):
        kind = k % 16
        t = "lookup" if kind < 8 else SPECIAL_TAG[(k // 16) % 4] if kind == 8 else BASE_TAG[kind]
        add("base", K.frame(rng, k, rt, len(rt)), t)

    for ntags in range(5):
        tags = K.TAGS[ntags]
        l3 = 14 + 4 * ntags
        whole = M.eth(M.ETH_P_IPV6, ipv6(17, 64, r(8), r), tags)
        for n in range(l3, l3 + 44):
            add("v6", whole[:n], sem(ntags, 6, n))
        for rep in range(6):
            for hop in (0, 1, 2, 255):
                f = M.eth(M.ETH_P_IPV6, ipv6([17, 6, 58][rep % 3], hop, r(rep), r), tags)
                add("v6", f, sem(ntags, 6, len(f), ttl=hop))
    for rep in range(8):
        # seven chained headers (hop-by-hop, destination, routing, mobility, AH
        # and two more), eight bytes each: 96 bytes hold five and the sixth's
        # first two bytes, all that the loop's six rounds read
        chain = b"".join(bytes([nh, 0]) + r(6) for nh in (60, 43, 135, 51, 0, 60, 17))
        f = M.eth(M.ETH_P_IPV6, ipv6(0, 64, chain + r(8), r))[:MAXLEN]
        add("v6", f, ":68")
        f = M.eth(M.ETH_P_IPV6, ipv6(44, 64, bytes([17, 0]) + r(6) + r(8), r), K.TAGS[rep % 5])
        add("v6", f, ":126/6")                          # a fragment header: walked (frags_ok)
        f = M.eth(M.ETH_P_IPV6, ipv6(44, 64, bytes([17]), r), K.TAGS[rep % 5])
        add("v6", f, ":68")                             # and one that does not fit

    for rep, dst in enumerate(DST_OK):
        for ntags in range(5):
            for le in LE_CHECKS:
                for ttl in (2, 255):
                    add("check", v4(dst, K.TAGS[ntags], ttl=ttl, payload=r(rep),
                                    check=int.from_bytes(le.to_bytes(2, "little"), "big")), ":123")

    for ntags in (0, 4):
        l3 = 14 + 4 * ntags
        for ihl in range(16):
            f = v4(DST_OK[ihl % 5], K.TAGS[ntags], ihl=ihl, payload=r(4))
            for n in (l3 + max(20, 4 * ihl), l3 + max(20, 4 * ihl) - 1):
                add("ihl", f[:n], sem(ntags, 4, n, ihl))

    for ntags in range(3):
        for fam in (4, 6):
            for n in (14, 17, 18, 33, 34):
                for rep in range(2):
                    f = v4(DST_OK[rep], K.TAGS[ntags], payload=r(30)) if fam == 4 else \
                        M.eth(M.ETH_P_IPV6, ipv6(17, 64, r(8), r), K.TAGS[ntags])
                    add("short", f[:n], sem(ntags, fam, n))

    for k in range(96):
        add("absent", v4(NET_ABSENT_B | int(rng.integers(1 << 16)), K.TAGS[k % 5], ttl=2 + k, payload=r(k % 9)),
            ":114")
    for k in range(32):     # more for the first: the slot-126 ifindex under every tag depth
        add("absent", v4(NET_ABSENT_A | int(rng.integers(1 << 16)), K.TAGS[k % 5], payload=r(k % 9)), ":114")

    cols = [np.array([len(f) for f in frames], np.uint32), np.array(part, np.uint8), np.array(tag, np.uint8)]
    for a in cols:
        a.setflags(write=False)
    return Corpus(tuple(frames), *cols)


@functools.lru_cache(maxsize=None)
def slots():
    """The corpus in MAXLEN-byte slots, in corpus order: (data u8[n, MAXLEN],
    lens u32[n]), read-only; zeros behind a frame."""
    c = corpus()
    data = np.zeros((len(c.frames), MAXLEN), np.uint8)
    for i, f in enumerate(c.frames):
        data[i, :len(f)] = np.frombuffer(f, np.uint8)
    data.setflags(write=False)
    return data, c.lens


def dump(path, table=8):
    """The corpus with a table's FIB and ports as the batch file the stand-alone
    sanitizer program of oracle/ref/ref_forward_harness.c reads."""
    import xftools as X
    data, lens = slots()
    r, nh, macs = X.forward_tables(routes(), nexthops(table))
    ports = np.asarray(ifindexes(table), np.uint32)
    with open(path, "wb") as f:
        f.write(np.array([0x46574452, len(lens), MAXLEN, len(r), len(nh), len(ports)], np.uint32).tobytes())
        for a in (lens, data, r, nh, macs, ports):
            f.write(np.ascontiguousarray(a).tobytes())


@functools.lru_cache(maxsize=None)
def permuted():
    """(fid, v): a permutation of the corpus and verdicts with about 60 % PASS,
    the pattern of the GPU tests."""
    rng = np.random.default_rng(60)
    n = len(corpus().frames)
    fid = rng.permutation(n)
    v = K.OTHERS[rng.integers(0, len(K.OTHERS), n)]
    v[rng.random(n) < 0.6] = M.PASS
    for a in (fid, v):
        a.setflags(write=False)
    return fid, v


NCHECK = 65536


@functools.lru_cache(maxsize=None)
def check_slots():
    """(data u8[65536, 64], lens): routed IPv4 frame k stores check k as a
    little-endian load of the field sees it, under k % 5 tags, with TTL 2 + k %
    254 and an ident chosen so that the header's checksum is valid."""
    k = np.arange(NCHECK)
    data = np.zeros((NCHECK, 64), np.uint8)
    lens = np.zeros(NCHECK, np.uint32)
    for ntags in range(5):
        rows = k[k % 5 == ntags]
        l3 = 14 + 4 * ntags
        head = M.eth(M.ETH_P_IP, b"", K.TAGS[ntags])
        data[rows, :l3] = np.frombuffer(head, np.uint8)
        h = np.zeros((len(rows), 20), np.uint8)
        h[:, 0], h[:, 1], h[:, 3] = 0x45, rows & 0xff, 20
        h[:, 8], h[:, 9] = 2 + rows % 254, 17
        h[:, 10], h[:, 11] = rows & 0xff, rows >> 8
        h[:, 12:16] = [192, 0, 2, 1]
        dst = np.array(DST_OK, np.uint32)[(rows // 5) % 5]
        for b in range(4):
            h[:, 16 + b] = (dst >> (24 - 8 * b)) & 0xff
        s = (h[:, 0::2].astype(np.uint32) << 8 | h[:, 1::2]).sum(axis=1)
        s = (s & 0xffff) + (s >> 16)
        s = (s & 0xffff) + (s >> 16)
        ident = 0xffff - s              # s + ident == 0xffff: the header sums to all ones
        h[:, 4], h[:, 5] = ident >> 8, ident & 0xff
        data[rows, l3:l3 + 20] = h
        lens[rows] = l3 + 20
    data.setflags(write=False)
    lens.setflags(write=False)
    return data, lens

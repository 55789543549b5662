"""Frames for the tests against the reference's own programs (oracle/ref/).

tools/xfsynth.c's fuzz generator was written beside the kernels; this corpus
is independent of it: pure Python over pktbuild.py, seeded, enumerating the
edges of headers/xdp/parsing_helpers.h and xdp-filter/xdpfilt_prog.h one
category at a time.  Every frame is at most MAXLEN bytes.

Categories (CATS; corpus() returns each frame's category):
  trunc  every tests/kat.py frame cut at every length 0..len
  byte   every distinct kat.py frame, every byte offset below 80, the byte
         replaced by each of BYTE_VALUES that changes it
  vlan   0-6 tags in every mix of 0x8100 / 0x88a8 (VLAN_MAX_DEPTH is 4; the
         inner type is read after the loop), whole and cut inside the tags
  ipv4   ihl 0-15 against frames that do and do not hold ihl*4 bytes; MF,
         offset, both; total_len lies
  ipv6   extension chains of 0-7 headers (hop-by-hop, destination, routing,
         mobility, fragment, AH, NONE) around IPV6_EXT_MAX_CHAIN = 6; header
         lengths that put the next header beside the kernels' 64- and
         128-byte window edges; lengths past the frame end
  icmp6  types 133-137; NS / NA with the target whole, cut at each of its 16
         bytes, and behind an extension chain
  udp    len 0-9 and larger than the frame
  tcp    doff 0-15 against frames that end before and after doff*4
  arp    hrd / pro / hln / pln wrong in turn; op 0-3; cut at each length;
         under 1-2 VLAN tags
  runt   frames of 0-13 bytes over the ruled and unruled MACs (parse_ethhdr's
         only failure; the Ethernet-only programs abort nothing else)

Window edges: with 14 + 4*tags bytes of Ethernet and 40 of IPv6, and
extension headers of 8*k or (AH) 4*k bytes, a next header starts at an
offset = 2 mod 4, never at byte 64 or 128 nor one beside them.  The nearest
on both sides are used: 62 / 66 / 70 and 126 / 130 / 134, so that an 8-byte
UDP header or TCP's doff byte straddles or just clears the edge.

Addresses, MACs and ports of the generated categories come from the pools
below; rules() flags them so that roughly half the lookups hit, src-only,
dst-only and both mixed, on top of kat.kat_rules() for the kat-derived rows.
"""
from __future__ import annotations

import functools
import itertools
import struct

import numpy as np

import kat
import pktbuild as P

MAXLEN = 160
SEED = 20260

CATS = ["trunc", "byte", "vlan", "ipv4", "ipv6", "icmp6", "udp", "tcp", "arp", "runt"]
# EtherType halves; IP protocol / next-header numbers (ICMP 1, TCP 6, UDP 17,
# routing 43, fragment 44, ESP 50, AH 51, ICMPv6 58, NONE 59, dstopts 60,
# mobility 135, NA 136); IPv4/IPv6 version+ihl bytes; small numbers.
BYTE_VALUES = sorted({0x08, 0x00, 0x06, 0x86, 0xdd, 0x81, 0x88, 0xa8,
                      1, 6, 17, 43, 44, 50, 51, 58, 59, 60, 135, 136,
                      0x45, 0x46, 0x4f, 0x40, 0x60,
                      0, 1, 4, 5, 6, 15, 255})

SRC, DST, TCPF, UDPF = 1, 2, 4, 8
# pool index -> rule flags (None: no rule; 4: a key that is present and never
# matches an address lookup, CHECK_MAP's mask test)
POOL_FLAGS = [SRC, DST, SRC | DST, 4, None, None, DST, SRC]
MACS = [bytes([0x02, 0xaa, 0, 0, 0, i]) for i in range(1, 9)]
V4 = ["10.77.0.%d" % i for i in range(1, 9)]
V6 = ["2001:db8:77::%x" % i for i in range(1, 9)]
PORTS = [1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008]
PORT_FLAGS = [DST | TCPF | UDPF, SRC | TCPF | UDPF, DST | UDPF, DST | TCPF,
              SRC | DST | TCPF | UDPF, None, None, SRC]   # (SRC alone: no protocol bit, never hits)
# MAC choice for the generated categories: mostly unruled, so that the
# programs with the Ethernet feature still parse most frames further
MAC_WEIGHTS = np.array([1, 1, 1, 1, 6, 6, 1, 1], float) / 18


def rules():
    """kat.kat_rules() plus the pools' rules (pre-existing hit counts on some)."""
    rs = kat.kat_rules()

    def add(keys, vals, pool, packer):
        k = [list(packer(a)) for a, f in zip(pool, POOL_FLAGS) if f is not None]
        v = [f | (i << 6) for i, f in enumerate(f for f in POOL_FLAGS if f is not None)]
        return (np.vstack([keys, np.array(k, np.uint8)]),
                np.concatenate([vals, np.array(v, np.uint64)]))

    rs.v4_keys, rs.v4_vals = add(rs.v4_keys, rs.v4_vals, V4, P.ip4)
    rs.v6_keys, rs.v6_vals = add(rs.v6_keys, rs.v6_vals, V6, P.ip6)
    rs.eth_keys, rs.eth_vals = add(rs.eth_keys, rs.eth_vals, MACS, bytes)
    for p, f in zip(PORTS, PORT_FLAGS):
        if f is not None:
            rs.ports[kat.port_key(p)] = f
    return rs


class _Gen:
    def __init__(self):
        self.rng = np.random.default_rng(SEED)
        self.frames: list[bytes] = []
        self.lens: list[int] = []
        self.cats: list[int] = []

    def add(self, cat, frame, cut=None):
        """A frame, or its first `cut` bytes: the rest stays behind it in the
        slot, where no program may look (the frame ends at its length)."""
        assert len(frame) <= MAXLEN, (cat, len(frame))
        self.frames.append(bytes(frame))
        self.lens.append(len(frame) if cut is None else max(0, min(cut, len(frame))))
        self.cats.append(CATS.index(cat))

    def pick(self, pool):
        return pool[int(self.rng.integers(0, len(pool)))]

    def eth(self, ethertype, vlans=()):
        d, s = self.rng.choice(8, 2, p=MAC_WEIGHTS)
        return P.eth(MACS[d], MACS[s], ethertype, vlans)

    def v4(self, proto, payload, **kw):
        return P.ipv4(self.pick(V4), self.pick(V4), proto, payload=payload, **kw)

    def v6(self, nh, payload):
        return P.ipv6(self.pick(V6), self.pick(V6), nh, payload)

    def udp(self, **kw):
        return P.udp(self.pick(PORTS), self.pick(PORTS), **kw)

    def tcp(self, **kw):
        return P.tcp(self.pick(PORTS), self.pick(PORTS), **kw)

    def l4(self, proto):
        return self.udp() if proto == 17 else self.tcp()


EXT_KINDS = {0: "opt", 60: "opt", 43: "opt", 135: "opt", 44: "frag", 51: "ah"}


def _chain(types, final, hdrlens=None):
    """Extension headers of the given next-header numbers ending in `final`;
    returns (first next-header, bytes).  59 (NONE) is no extension header: the
    walk stops at it, whatever follows."""
    b = b""
    for i, t in enumerate(types):
        nxt = types[i + 1] if i + 1 < len(types) else final
        hl = hdrlens[i] if hdrlens else 0
        b += P.ext(nxt, hl, EXT_KINDS.get(t, "opt"))
    return (types[0] if types else final), b


def _trunc(g):
    for _, fr, _ in kat.kat_frames():
        for n in range(len(fr) + 1):
            g.add("trunc", fr, n)


def _byte(g):
    seen = set()
    for _, fr, _ in kat.kat_frames():
        if fr in seen or not fr:
            continue
        seen.add(fr)
        for off in range(min(80, len(fr))):
            for v in BYTE_VALUES:
                if fr[off] != v:
                    g.add("byte", fr[:off] + bytes([v]) + fr[off + 1:])


def _vlan(g):
    for depth in range(7):
        for tpids in itertools.product((0x8100, 0x88a8), repeat=depth):
            tags = [(t, 5) for t in tpids]
            for et, l3 in ((0x0800, lambda: g.v4(17, g.udp())),
                           (0x86DD, lambda: g.v6(6, g.tcp())),
                           (0x0806, lambda: P.arp(1, sip=g.pick(V4), tip=g.pick(V4)))):
                fr = g.eth(et, tags) + l3()
                g.add("vlan", fr)
                # cut inside each tag, and right behind the tags
                for cut in {14 + 4 * d + k for d in range(depth + 1) for k in (0, 2)}:
                    g.add("vlan", fr, cut)


def _ipv4(g):
    for ihl in range(16):
        for proto in (17, 6, 1):
            pay = g.l4(proto) if proto != 1 else P.icmp4_echo()
            fr = bytearray(g.eth(0x0800) + g.v4(proto, pay, ihl=max(ihl, 5)))
            fr[14] = 0x40 | ihl            # (ihl < 5: the header bytes stay, L4 is read inside them)
            fr = bytes(fr)
            g.add("ipv4", fr)
            for cut in (14 + 19, 14 + 20, 14 + ihl * 4 - 1, 14 + ihl * 4, 14 + ihl * 4 + 7,
                        14 + ihl * 4 + 8, 14 + ihl * 4 + 19, 14 + ihl * 4 + 20):
                if 14 <= cut < len(fr):
                    g.add("ipv4", fr, cut)
    for frag in (0x2000, 0x0001, 0x1fff, 0x2001, 0x3fff, 0x0000, 0x8000):
        for proto in (17, 6):
            g.add("ipv4", g.eth(0x0800) + g.v4(proto, g.l4(proto), frag=frag))
            g.add("ipv4", g.eth(0x0800, [(0x8100, 9)]) + g.v4(proto, g.l4(proto), frag=frag, ihl=6))
    for tl in (0, 1, 19, 20, 27, 28, 29, 1500, 65535):
        for proto in (17, 6):
            g.add("ipv4", g.eth(0x0800) + g.v4(proto, g.l4(proto), total_len=tl))


def _ipv6(g):
    kinds = [0, 60, 43, 135, 44, 51]
    # chains of 0-7 headers: every single type repeated, and seeded mixes
    # (some with NONE inside: the walk returns 59 there)
    for n in range(8):
        mixes = [[k] * n for k in kinds] if n else [[]]
        for _ in range(12 if n else 0):
            mixes.append([int(g.rng.choice(kinds + [59])) for _ in range(n)])
        for types in mixes:
            for final in (17, 6, 58, 59):
                nh, ext = _chain(types, final)
                pay = g.l4(final) if final in (17, 6) else P.icmp6(128) if final == 58 else b""
                fr = g.eth(0x86DD) + g.v6(nh, ext + pay)
                g.add("ipv6", fr)
                g.add("ipv6", fr, len(fr) - len(pay) + 1)     # one byte of the last header
                g.add("ipv6", fr, len(fr) - len(pay) - 1)     # cut inside the last extension
    # next header beside the window edges (module docstring): option headers
    # of 8, 16, 24 bytes after 54 -> 62, 66 (AH 12), 70; 72 + ... -> 126, 130, 134
    edges = [([0], [0], 62), ([51], [1], 66), ([60], [1], 70),
             ([0], [8], 126), ([51], [17], 130), ([43], [9], 134),
             ([0, 60], [3, 4], 126), ([0, 51], [7, 1], 130)]
    for types, hls, at in edges:
        for final in (17, 6, 58):
            nh, ext = _chain(types, final, hls)
            assert 54 + len(ext) == at
            pay = g.l4(final) if final != 58 else P.ndisc_ns(g.pick(V6))
            fr = g.eth(0x86DD) + g.v6(nh, ext + pay)
            for cut in (at - 1, at, at + 1, at + 2, at + 7, at + 8, at + 13, at + 14, len(fr)):
                g.add("ipv6", fr, cut)
        # the same under one VLAN tag: 4 bytes further
        nh, ext = _chain(types, 17, hls)
        if 58 + len(ext) + 16 <= MAXLEN:
            g.add("ipv6", g.eth(0x86DD, [(0x88a8, 3)]) + g.v6(nh, ext + g.udp()))
    # header lengths that point past the frame end
    for t in kinds:
        for hl in (1, 2, 12, 13, 31, 128, 255):
            nh, ext = _chain([t], 17)
            ext = bytes([ext[0], hl]) + ext[2:]
            g.add("ipv6", g.eth(0x86DD) + g.v6(nh, ext + g.udp()))
            g.add("ipv6", g.eth(0x86DD) + g.v6(nh, ext + g.udp(payload=b"y" * 90)))


def _icmp6(g):
    for typ in (133, 134, 135, 136, 137):
        for tgt in V6:
            body = P.icmp6(typ, 0, P.ip6(tgt))
            g.add("icmp6", g.eth(0x86DD) + g.v6(58, body))
    for typ in (135, 136):
        for tgt in V6:
            fr = g.eth(0x86DD) + g.v6(58, P.icmp6(typ, 0, P.ip6(tgt)))
            for cut in range(17):          # the 8-byte ICMPv6 header, then 0..16 target bytes
                g.add("icmp6", fr, 54 + 8 + cut)
            for cut in range(8):           # inside the ICMPv6 header
                g.add("icmp6", fr, 54 + cut)
            for types in ([0], [60, 43], [0, 60, 43, 135, 51], [0] * 6, [44]):
                nh, ext = _chain(types, 58)
                fr2 = g.eth(0x86DD) + g.v6(nh, ext + P.icmp6(typ, 0, P.ip6(tgt)))
                g.add("icmp6", fr2)
                g.add("icmp6", fr2, len(fr2) - 1)


def _udp(g):
    for ln in list(range(10)) + [50, 1400, 65535]:
        for _ in range(6):
            g.add("udp", g.eth(0x0800) + g.v4(17, g.udp(length=ln)))
            g.add("udp", g.eth(0x86DD) + g.v6(17, g.udp(length=ln)))
        for cut in range(1, 9):
            fr = g.eth(0x0800) + g.v4(17, g.udp(length=ln))
            g.add("udp", fr, 34 + cut - 1)


def _tcp(g):
    for doff in range(16):
        for v6 in (False, True):
            for _ in range(4):
                seg = g.tcp(doff=max(doff, 5))
                seg = seg[:12] + bytes([doff << 4]) + seg[13:]
                fr = (g.eth(0x86DD) + g.v6(6, seg)) if v6 else (g.eth(0x0800) + g.v4(6, seg))
                l4 = 54 if v6 else 34
                g.add("tcp", fr)
                for cut in (l4 + 19, l4 + 20, l4 + doff * 4 - 1, l4 + doff * 4, l4 + doff * 4 + 1):
                    if l4 <= cut <= len(fr):
                        g.add("tcp", fr, cut)


def _arp(g):
    def arp(op=1, **kw):
        return P.arp(op, sha=g.pick(MACS), sip=g.pick(V4), tha=g.pick(MACS), tip=g.pick(V4), **kw)

    for op in range(4):
        for _ in range(24):
            g.add("arp", g.eth(0x0806) + arp(op))
        for tags in ([(0x8100, 1)], [(0x88a8, 1), (0x8100, 2)]):
            for _ in range(8):
                g.add("arp", g.eth(0x0806, tags) + arp(op))
    for bad in (dict(hrd=0), dict(hrd=6), dict(hrd=0x0100), dict(pro=0x86DD), dict(pro=0x0008),
                dict(hln=0), dict(hln=5), dict(hln=8), dict(pln=0), dict(pln=16), dict(pln=6)):
        for op in (1, 2):
            for _ in range(4):
                g.add("arp", g.eth(0x0806) + arp(op, **bad))
    for op in (1, 2):
        for _ in range(3):
            fr = g.eth(0x0806) + arp(op)
            for cut in range(14, len(fr)):
                g.add("arp", fr, cut)
            g.add("arp", fr + b"\0" * 18)      # padded to the Ethernet minimum


def _runt(g):
    behind = [lambda: (0x0800, g.v4(17, g.udp())), lambda: (0x0800, g.v4(6, g.tcp())),
              lambda: (0x86DD, g.v6(17, g.udp())), lambda: (0x86DD, g.v6(58, P.ndisc_ns(g.pick(V6)))),
              lambda: (0x0806, P.arp(1, sip=g.pick(V4), tip=g.pick(V4))), lambda: (0x88CC, b""),
              lambda: (0x8100, struct.pack("!HH", 7, 0x0800) + g.v4(17, g.udp())),
              lambda: (0x88a8, struct.pack("!HH", 7, 0x86DD) + g.v6(6, g.tcp()))]
    for d in range(8):
        for s in range(8):
            for mk in behind:       # a whole frame of each kind behind the cut
                et, l3 = mk()
                fr = P.eth(MACS[d], MACS[s], et) + l3
                for n in range(15):
                    g.add("runt", fr, n)


@functools.lru_cache(maxsize=None)
def corpus():
    """(frames, lens, cats): a tuple of slot contents, and read-only arrays of
    each frame's length (a cut frame's slot holds the uncut bytes behind it)
    and of its index into CATS.  Built once; do not modify."""
    g = _Gen()
    for fn in (_trunc, _byte, _vlan, _ipv4, _ipv6, _icmp6, _udp, _tcp, _arp, _runt):
        fn(g)
    lens, cats = np.array(g.lens, np.uint32), np.array(g.cats, np.uint8)
    lens.setflags(write=False)
    cats.setflags(write=False)
    return tuple(g.frames), lens, cats


@functools.lru_cache(maxsize=None)
def slots(stride=MAXLEN):
    """The corpus in `stride`-byte slots, in corpus order: (data u8[n, stride],
    lens u32[n]), read-only.  A frame longer than the slot is cut to it."""
    frames, lens, _ = corpus()
    data = np.zeros((len(frames), stride), np.uint8)
    for i, fr in enumerate(frames):
        fr = fr[:stride]
        data[i, :len(fr)] = np.frombuffer(fr, np.uint8)
    lens = np.minimum(lens, stride).astype(np.uint32)
    data.setflags(write=False)
    lens.setflags(write=False)
    return data, lens


def pack(idx, stride=MAXLEN):
    """The frames `idx` (corpus indices, any order, repeats allowed) as a
    fixed-stride batch: (data u8[len(idx)*stride], lens u32)."""
    data, lens = slots(stride)
    return np.ascontiguousarray(data[idx]).reshape(-1), np.ascontiguousarray(lens[idx])


def pack_offsets(idx, seed=SEED):
    """The frames `idx` back to back at their own lengths with seeded gaps of
    0-7 bytes (unaligned starts): (data, offsets u64, lens u32)."""
    data, lens = slots(MAXLEN)
    lens = np.ascontiguousarray(lens[idx])
    rng = np.random.default_rng(seed)
    gaps = rng.integers(0, 8, len(idx)).astype(np.uint64)
    l64 = lens.astype(np.uint64)
    offs = np.cumsum(l64 + gaps) - l64
    out = np.zeros(int(offs[-1] + l64[-1]) + 256, np.uint8)
    for o, i, n in zip(offs.tolist(), np.asarray(idx).tolist(), lens.tolist()):
        out[o:o + n] = data[i, :n]
    return out, offs, lens


def fits64():
    """Indices of the corpus frames of at most 64 bytes (the W=64 kernels)."""
    return np.nonzero(corpus()[1] <= 64)[0]


def tiled(idx, at_least, seed=SEED):
    """`idx` repeated under a fresh seeded permutation each time until at
    least `at_least` frames, the last repeat cut so that the total is 37 past
    a multiple of 64: every frame at many lane and tile positions, beside
    different neighbours, and a ragged last tile."""
    rng = np.random.default_rng(seed)
    n = max(len(idx), at_least)
    total = n + (37 - n) % 64
    out = [np.asarray(idx)]
    while sum(map(len, out)) < total:
        out.append(rng.permutation(idx))
    return np.concatenate(out)[:total]

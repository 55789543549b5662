"""Frames for the tests of steered egress against the reference's own
redirect-cpu programs (oracle/ref/ref_cpumap_harness.c).

Seeded and deterministic, built from steermodel.py's frame builders; every
frame is at most MAXLEN bytes.  A cut frame keeps its uncut bytes behind it in
its slot (as refcorpus.py's do): a kernel that ignored a frame's length would
read a plausible header there and choose a plausible, wrong queue.

Parts (PARTS; corpus().part is each frame's index into it):
  cut        every shape {IPv4, IPv6} x {TCP, UDP, ICMP / ICMPv6} x STACKS (0-3
             VLAN tags, both TPIDs, mixed), and ARP under 0-2 tags, cut at every
             length 0..len
  ethertype  the ethertype's high byte 0x00-0xff with low bytes 0x00 and 0xff
             (0x05ff / 0x0600 among them) and the known types, over an IPv4 and
             an IPv6 UDP frame, whole and one byte short
  proto      every IPv4 protocol and IPv6 nexthdr value 0-255 in front of a
             TCP header (IPv6 also behind two tags), whole and one byte short
  ihl        ihl 0-15 over UDP and TCP, whole and one byte short: the programs
             read the ports at l3 + 20 whatever ihl says
  ext        an IPv6 extension header (hop-by-hop, routing, fragment, ESP, AH,
             destination, mobility, NONE) in front of a UDP header: the
             programs do not walk extension headers, the port is 0
  addr       address pairs whose 32-bit sums wrap, all-ones and all-zero
             addresses, swapped pairs, IPv6 pairs that differ in one word,
             against ports 0, 1, 0x00ff, 0xff00 and 0xffff on both sides
  flow       whole frames of random flows (the spread over 64 queues)
  hand       steermodel.hand_rows()
  other      a seeded sample of tests/refcorpus.py

Tags (TAGS; corpus().tag): what the reference's programs do with the frame,
known from how the frame was built, one tag a return statement of parse_eth,
get_*_hash_ip_pair, get_proto_* and get_port_* that cpumap_l4_hash / _sport /
_dport can reach (":N" are lines of xdp-bench/xdp_redirect_cpumap.bpf.c).
test_steer_reference.py asserts the reference's result per tag (EXPECT):
  eth_short  below 14 bytes (:62)                            refused
  eth_802_3  ethertype below 0x0600 (:68)                    refused
  tag1_cut   cut inside the first tag (:78)                  refused
  tag2_cut   cut inside the second tag (:89)                 refused
  tag3       a third tag: a VLAN ethertype is left (:95, then :548, :626)   key 0
  l3_other   ARP and every other ethertype (:548, :626)      key 0
  ip4_cut    cut inside the IPv4 header (:199, :478)         key 0
  ip6_cut    cut inside the IPv6 header (:211, :495)         key 0
  ip4_other, ip6_other   a whole header, neither TCP nor UDP (:200 / :212,
             :609 / :622; hashed, :483 / :503)               port 0
  udp4_cut, tcp4_cut, udp6_cut, tcp6_cut   the L4 header does not fit
             (:113, :159, :136, :182)                        port 0
  udp4, tcp4, udp6, tcp6   the port is read (:116 / :118, :162 / :164,
             :139 / :141, :185 / :187)                       port = sport / dport
  any        no statement (the hand rows have their own table; the other
             frames are not ours)
get_port_*'s first two returns (:107 / :109 and their likes) cannot be reached
from these three programs: get_proto_* has seen the whole header and that
protocol before get_port_* is called.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import refcorpus as R
import steermodel as M

MAXLEN = 160
SEED = 6324
Q, AD = M.ETH_P_8021Q, M.ETH_P_8021AD

PARTS = ["cut", "ethertype", "proto", "ihl", "ext", "addr", "flow", "hand", "other"]
TAGS = ["eth_short", "eth_802_3", "tag1_cut", "tag2_cut", "tag3", "l3_other", "ip4_cut", "ip6_cut",
        "ip4_other", "ip6_other", "udp4_cut", "tcp4_cut", "udp6_cut", "tcp6_cut",
        "udp4", "tcp4", "udp6", "tcp6", "any"]
# tag -> what the reference must answer: "refused"; "zero" (not refused, key 0
# in every mode); "port0" (not refused, key 0 in SPORT and DPORT); "port" (not
# refused, the key is the frame's sport / dport); None
EXPECT = dict(eth_short="refused", eth_802_3="refused", tag1_cut="refused", tag2_cut="refused",
              tag3="zero", l3_other="zero", ip4_cut="zero", ip6_cut="zero",
              ip4_other="port0", ip6_other="port0", udp4_cut="port0", tcp4_cut="port0",
              udp6_cut="port0", tcp6_cut="port0", udp4="port", tcp4="port", udp6="port", tcp6="port",
              any=None)
STACKS = [(), (Q,), (AD,), (Q, Q), (AD, AD), (AD, Q), (Q, AD), (Q, Q, Q), (AD, Q, AD)]
PORTS5 = (0, 1, 0x00ff, 0xff00, 0xffff)
EXT_NEXTHDRS = (0, 43, 44, 50, 51, 60, 135, 59)
N_OTHER, N_FLOWS = 3000, 1536


def sem(ntags, l3, l4, n):
    """The tag of the first @n bytes of a frame built as Ethernet, @ntags VLAN
    tags, an @l3 header ("v4", "v6", anything else) and an @l4 header ("tcp",
    "udp", anything else)."""
    if n < 14:
        return "eth_short"
    if ntags >= 1 and n < 18:
        return "tag1_cut"
    if ntags >= 2 and n < 22:
        return "tag2_cut"
    if ntags >= 3:
        return "tag3"
    if l3 not in ("v4", "v6"):
        return "l3_other"
    fam = l3[1]
    at = 14 + 4 * ntags + (20 if fam == "4" else 40)
    if n < at:
        return f"ip{fam}_cut"
    if l4 not in ("tcp", "udp"):
        return f"ip{fam}_other"
    if n < at + (20 if l4 == "tcp" else 8):
        return f"{l4}{fam}_cut"
    return f"{l4}{fam}"


class Corpus(NamedTuple):
    frames: tuple           # slot contents: the uncut bytes
    lens: np.ndarray        # u32: the frame is the slot's first lens[i] bytes
    part: np.ndarray        # u8 index into PARTS
    tag: np.ndarray         # u8 index into TAGS
    sport: np.ndarray       # u16: the ports a "port" frame was built with
    dport: np.ndarray
    qinq6: np.ndarray       # indices of the cut part's double-tagged IPv6 TCP / UDP frames


class _Gen:
    def __init__(self):
        self.rng = np.random.default_rng(SEED)
        self.frames, self.lens, self.part, self.tag, self.sport, self.dport = [], [], [], [], [], []
        self.qinq6 = []

    def add(self, part, frame, tag, cut=None, sp=0, dp=0):
        assert len(frame) <= MAXLEN, (part, len(frame))
        self.frames.append(bytes(frame))
        self.lens.append(len(frame) if cut is None else cut)
        self.part.append(PARTS.index(part))
        self.tag.append(TAGS.index(tag))
        port = EXPECT[tag] == "port"
        self.sport.append(sp if port else 0)
        self.dport.append(dp if port else 0)

    def r(self, k):
        return bytes(self.rng.integers(0, 256, k, dtype=np.uint8))

    def port(self):
        return int(self.rng.integers(1, 65536))

    def shape(self, l3, l4, stack, sp, dp, pay=b"", proto=None, sa=None, da=None, **kw):
        """Ethernet / @stack / @l3 / @l4 with random addresses."""
        n = 4 if l3 == "v4" else 16
        sa, da = sa or self.r(n), da or self.r(n)
        if l4 == "tcp":
            seg, p = M.tcp(sp, dp, pay), 6
        elif l4 == "udp":
            seg, p = M.udp(sp, dp, pay), 17
        else:
            seg, p = bytes(8) + pay, 1 if l3 == "v4" else 58
        p = p if proto is None else proto
        if l3 == "v4":
            return M.eth(M.ETH_P_IP, M.ipv4(sa, da, p, seg, **kw), stack)
        return M.eth(M.ETH_P_IPV6, M.ipv6(sa, da, p, seg), stack)


def _cut(g):
    for stack in STACKS:
        for l3 in ("v4", "v6"):
            for l4 in ("tcp", "udp", "icmp"):
                sp, dp = g.port(), g.port()
                fr = g.shape(l3, l4, stack, sp, dp, g.r(6))
                for n in range(len(fr) + 1):
                    if l3 == "v6" and l4 != "icmp" and len(stack) == 2:
                        g.qinq6.append(len(g.frames))
                    g.add("cut", fr, sem(len(stack), l3, l4, n), n, sp, dp)
    for stack in ((), (Q,), (AD, Q)):
        fr = M.eth(0x0806, bytes([0, 1, 8, 0, 6, 4, 0, 1]) + g.r(20), stack)
        for n in range(len(fr) + 1):
            g.add("cut", fr, sem(len(stack), "arp", None, n), n)


def _whole_and_short(g, part, fr, ntags, l3, l4, sp, dp):
    g.add(part, fr, sem(ntags, l3, l4, len(fr)), None, sp, dp)
    g.add(part, fr, sem(ntags, l3, l4, len(fr) - 1), len(fr) - 1, sp, dp)


def _ethertype(g):
    types = [hi << 8 | lo for hi in range(256) for lo in (0x00, 0xff)] + [AD, M.ETH_P_IPV6, 0x0806]
    for l3, own in (("v4", M.ETH_P_IP), ("v6", M.ETH_P_IPV6)):
        for e in types:
            sp, dp = g.port(), g.port()
            base = g.shape(l3, "udp", (), sp, dp)
            fr = base[:12] + e.to_bytes(2, "big") + base[14:]
            # as a tag, an IP header's bytes 2..3 are the inner type: the
            # total length (0x001c) or flow-label zeros, never checked again
            # against 0x0600 and no type the programs know
            assert fr[16:18] in (b"\x00\x1c", b"\x00\x00")
            for n in (len(fr), len(fr) - 1):
                if e < 0x0600:
                    tag = "eth_802_3"
                elif e == own:
                    tag = sem(0, l3, "udp", n)
                elif e in (M.ETH_P_IP, M.ETH_P_IPV6):
                    tag = "any"         # the other family's header read as this one
                else:
                    tag = "l3_other"    # (0x8100 / 0x88a8: one tag, inner type unknown)
                g.add("ethertype", fr, tag, n, sp, dp)


def _proto(g):
    for l3, stack in (("v4", ()), ("v6", ()), ("v6", (AD, Q))):
        for p in range(256):
            sp, dp = g.port(), g.port()
            fr = g.shape(l3, "tcp", stack, sp, dp, proto=p)
            l4 = {6: "tcp", 17: "udp"}.get(p)
            _whole_and_short(g, "proto", fr, len(stack), l3, l4, sp, dp)


def _ihl(g):
    for ihl in range(16):
        for l4 in ("udp", "tcp"):
            for stack in ((), (Q,)):
                sp, dp = g.port(), g.port()
                # (a reader honouring ihl = 6 would find other bytes at l3 + 24)
                fr = g.shape("v4", l4, stack, sp, dp, g.r(4), ihl=ihl)
                _whole_and_short(g, "ihl", fr, len(stack), "v4", l4, sp, dp)


def _ext(g):
    for nh in EXT_NEXTHDRS:
        for stack in ((), (Q,), (AD, Q)):
            sp, dp = g.port(), g.port()
            ext = bytes([17, 0]) + g.r(6)
            fr = M.eth(M.ETH_P_IPV6, M.ipv6(g.r(16), g.r(16), nh, ext + M.udp(sp, dp)), stack)
            _whole_and_short(g, "ext", fr, len(stack), "v6", None, sp, dp)


def _addr(g):
    ones4, zero4 = b"\xff" * 4, bytes(4)
    v4 = [(ones4, bytes([1, 0, 0, 0])), (ones4, bytes([0, 0, 0, 1])), (bytes([0, 0, 0, 0x80]),) * 2,
          (bytes([0xff, 0xff, 0, 0]), bytes([1, 0, 0, 0])), (ones4, ones4), (zero4, zero4),
          (zero4, ones4), (bytes([1, 2, 3, 4]), bytes([5, 6, 7, 8])), (g.r(4), g.r(4))]
    A6, B6 = bytes(range(1, 17)), bytes(range(101, 117))
    ones6, zero6 = b"\xff" * 16, bytes(16)
    v6 = [(ones6, ones6), (zero6, zero6), (zero6, ones6), (A6, B6), (g.r(16), g.r(16)),
          (ones6, bytes([1, 0, 0, 0] * 4)), (b"\xff\xff\xff\x7f" * 4, b"\x01\x00\x00\x80" * 4)]
    for w in range(4):       # pairs that differ in one word only
        v6.append((A6, A6[:4 * w] + bytes([0xee, w, 0, 0xee]) + A6[4 * w + 4:]))
    for l3, pairs in (("v4", v4), ("v6", v6)):
        pairs = pairs + [(b, a) for a, b in pairs if a != b]
        for k, (a, b) in enumerate(pairs):
            stack = () if l3 == "v4" else ((), (AD, Q))[k % 2]
            for sp in PORTS5:
                for dp in PORTS5:
                    for l4 in ("udp", "tcp"):
                        fr = g.shape(l3, l4, stack, sp, dp, sa=a, da=b)
                        g.add("addr", fr, sem(len(stack), l3, l4, len(fr)), None, sp, dp)


def _flow(g):
    for k in range(N_FLOWS):
        l3, l4 = ("v4", "v6")[(k // 2) % 2], ("udp", "tcp")[k % 2]
        stack = STACKS[int(g.rng.integers(0, 7))]
        sp, dp = g.port(), g.port()
        fr = g.shape(l3, l4, stack, sp, dp, g.r(k % 5))
        g.add("flow", fr, sem(len(stack), l3, l4, len(fr)), None, sp, dp)


def _hand(g):
    for _, fr in M.hand_rows():
        g.add("hand", fr, "any")


def _other(g):
    frames, lens, _ = R.corpus()
    for i in np.sort(g.rng.choice(len(frames), N_OTHER, replace=False)).tolist():
        g.add("other", frames[i][:MAXLEN], "any", min(int(lens[i]), MAXLEN))


@functools.lru_cache(maxsize=None)
def corpus() -> Corpus:
    """Built once; do not modify."""
    g = _Gen()
    for fn in (_cut, _ethertype, _proto, _ihl, _ext, _addr, _flow, _hand, _other):
        fn(g)
    cols = [np.array(g.lens, np.uint32), np.array(g.part, np.uint8), np.array(g.tag, np.uint8),
            np.array(g.sport, np.uint16), np.array(g.dport, np.uint16), np.array(g.qinq6, np.int64)]
    for a in cols:
        a.setflags(write=False)
    return Corpus(tuple(g.frames), *cols)


@functools.lru_cache(maxsize=None)
def slots():
    """The corpus in MAXLEN-byte slots, in corpus order: (data u8[n, MAXLEN],
    lens u32[n]), read-only.  A cut frame's slot holds its uncut bytes."""
    c = corpus()
    data = np.zeros((len(c.frames), MAXLEN), np.uint8)
    for i, fr in enumerate(c.frames):
        data[i, :len(fr)] = np.frombuffer(fr, np.uint8)
    data.setflags(write=False)
    return data, c.lens

"""A plain-Python/numpy model of xfg_steer_egress (include/xdpfilter_gpu.h): the
queue a PASS frame takes, the K-way order-preserving partition and the counts.

The queue choice follows xdp-bench redirect-cpu's programs; every rule names
the lines of the reference's xdp-bench/xdp_redirect_cpumap.bpf.c (":N" below)
or xdp-bench/hash_func01.h it models.  The citations are a reader's aid, not
the proof: tests/test_steer_reference.py holds queue_of_frame() equal to those
programs themselves, compiled for the host and run (oracle/ref/
ref_cpumap_harness.c), over tests/steercorpus.py and 100,000 random frames.
Frames are bytes objects; nothing here is fast, and nothing needs to be.
"""
import numpy as np

PASS = 2
L4_HASH, L4_SPORT, L4_DPORT = 0, 1, 2
QUEUE_NONE = 0xff
ADDR48 = (1 << 48) - 1
INITVAL = 15485863                      # :467
M32 = 0xffffffff
ETH_P_8021Q, ETH_P_8021AD, ETH_P_IP, ETH_P_IPV6 = 0x8100, 0x88a8, 0x0800, 0x86dd
IPPROTO_TCP, IPPROTO_UDP = 6, 17


def superfasthash4(x, initval):
    """SuperFastHash() of hash_func01.h over the four bytes of the u32 @x as a
    little-endian machine holds them (len 4: one turn of the main loop, :22-28,
    no tail, then the avalanche, :47-52)."""
    lo, hi = x & 0xffff, (x >> 16) & 0xffff
    h = (initval + lo) & M32                    # :23
    tmp = ((hi << 11) ^ h) & M32                # :24
    h = ((h << 16) ^ tmp) & M32                 # :25
    h = (h + (h >> 11)) & M32                   # :27
    h ^= (h << 3) & M32                         # :47
    h = (h + (h >> 5)) & M32
    h ^= (h << 4) & M32
    h = (h + (h >> 17)) & M32
    h ^= (h << 25) & M32
    h = (h + (h >> 6)) & M32                    # :52
    return h


def parse_eth(f):
    """parse_eth() (:53-96): (ethertype in host order, l3 offset), or None where
    it returns false."""
    n = len(f)
    off = 14
    if off > n:                                 # :61
        return None
    ty = f[12] << 8 | f[13]
    if ty < 0x0600:                             # :67
        return None
    for _ in range(2):                          # :71-80, :82-91
        if ty in (ETH_P_8021Q, ETH_P_8021AD):
            off += 4
            if off > n:                         # :77, :88
                return None
            ty = f[off - 2] << 8 | f[off - 1]
    return ty, off


def _le32(f, at):
    return int.from_bytes(f[at:at + 4], "little")


def key_of(f, mode):
    """What the program takes modulo cpus_count (:553, :629) -- the hash or the
    port -- or None for a frame parse_eth() refuses (:536-537, :594-595)."""
    p = parse_eth(f)
    if p is None:
        return None
    ty, l3 = p
    n = len(f)
    if ty == ETH_P_IP:
        if l3 + 20 > n:                         # :106, :152, :198, :477
            return 0
        proto = f[l3 + 9]
        if mode == L4_HASH:                     # :480-481
            s = (_le32(f, l3 + 12) + _le32(f, l3 + 16)) & M32
            return superfasthash4(s, (INITVAL + proto) & M32)
        l4 = l3 + 20                            # :111, :157: iph + 1, whatever ihl says
    elif ty == ETH_P_IPV6:
        if l3 + 40 > n:                         # :129, :175, :210, :494
            return 0
        proto = f[l3 + 6]
        if mode == L4_HASH:                     # :497-501
            s = sum(_le32(f, l3 + 8 + 4 * j) for j in range(8)) & M32
            return superfasthash4(s, (INITVAL + proto) & M32)
        l4 = l3 + 40                            # :134, :180: ip6h + 1, no extension headers
    else:
        return 0                                # :547-549, :625-626
    if proto == IPPROTO_TCP:                    # :602, :615
        if l4 + 20 > n:                         # :158, :181
            return 0
    elif proto == IPPROTO_UDP:                  # :605, :618
        if l4 + 8 > n:                          # :112, :135
            return 0
    else:
        return 0                                # :608-609, :621-622
    at = l4 if mode == L4_SPORT else l4 + 2     # :115-118
    return f[at] << 8 | f[at + 1]               # bpf_ntohs


def queue_of_frame(f, mode, avail, skip_queue):
    """(queue, refused) of one PASS frame: avail is cpus_available, its length
    cpus_count (:553-558, :629-634)."""
    k = key_of(f, mode)
    if k is None:
        return skip_queue, True
    return int(avail[k % len(avail)]), False


def steer_model(frames, addr, lens, v, nqueues, mode=L4_HASH, avail=None, skip_queue=0, fid=None):
    """frames[i]: record i's bytes [0, lens[i]) -- or, with @fid, frames a pool
    of frames and frames[fid[i]] record i's (each pool frame is parsed once).
    Returns (tx, fill, counts, queue_of): tx[q] the (k, 2) u64 TX records of
    queue q in order, fill the chunk addresses of the other records in order,
    counts the nqueues + 2 counts, queue_of the byte a record."""
    n = len(v)
    avail = list(range(nqueues)) if avail is None else list(avail)
    queue_of = np.full(n, QUEUE_NONE, np.uint8)
    passed = np.asarray(v) == PASS
    if fid is None:
        refused = 0
        for i in np.flatnonzero(passed):
            q, r = queue_of_frame(frames[i], mode, avail, skip_queue)
            queue_of[i] = q
            refused += r
    else:
        fid = np.asarray(fid, np.int64)
        per = [queue_of_frame(f, mode, avail, skip_queue) for f in frames]
        pq = np.array([q for q, _ in per], np.uint8)
        pr = np.array([r for _, r in per], bool)
        queue_of[passed] = pq[fid[passed]]
        refused = int(pr[fid[passed]].sum())
    addr = np.asarray(addr, np.uint64)
    lens = np.asarray(lens)
    tx = []
    for q in range(nqueues):
        m = queue_of == q
        r = np.empty((int(m.sum()), 2), np.uint64)
        r[:, 0] = addr[m]
        r[:, 1] = lens[m].astype(np.uint64)         # options 0
        tx.append(r)
    other = queue_of == QUEUE_NONE
    fill = addr[other] & np.uint64(ADDR48)
    counts = np.array([len(r) for r in tx] + [int(other.sum()), refused], np.uint64)
    return tx, fill, counts, queue_of


def walk(frames, addr, lens, v, nqueues, mode=L4_HASH, avail=None, skip_queue=0):
    """The same, record by record, as a consumer loop would do it."""
    avail = list(range(nqueues)) if avail is None else list(avail)
    tx = [[] for _ in range(nqueues)]
    fill, queue_of, refused = [], [], 0
    for i in range(len(v)):
        if v[i] != PASS:
            fill.append(int(addr[i]) & ADDR48)
            queue_of.append(QUEUE_NONE)
            continue
        k = key_of(frames[i], mode)
        if k is None:
            q = skip_queue
            refused += 1
        else:
            q = avail[k % len(avail)]
        tx[q].append((int(addr[i]), int(lens[i])))
        queue_of.append(q)
    return tx, fill, [len(t) for t in tx] + [len(fill), refused], queue_of


# ---- frames for the tests
def eth(ethertype, payload, tags=(), dst=b"\x02\x00\x00\x00\x00\x01", src=b"\x02\x00\x00\x00\x00\x02"):
    """An Ethernet frame: @tags the TPIDs of its VLAN tags, outermost first."""
    h = dst + src
    for k, tpid in enumerate(tags):
        h += tpid.to_bytes(2, "big") + (100 + k).to_bytes(2, "big")
    return h + ethertype.to_bytes(2, "big") + payload


def ipv4(saddr, daddr, proto, l4=b"", ihl=5):
    h = bytes([0x40 | ihl, 0]) + (20 + len(l4)).to_bytes(2, "big") + bytes(4) + bytes([64, proto]) + \
        bytes(2) + saddr + daddr
    return h + l4


def ipv6(saddr, daddr, nexthdr, l4=b""):
    return bytes([0x60, 0, 0, 0]) + len(l4).to_bytes(2, "big") + bytes([nexthdr, 64]) + saddr + daddr + l4


def udp(sport, dport, payload=b""):
    return sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (8 + len(payload)).to_bytes(2, "big") + \
        bytes(2) + payload


def tcp(sport, dport, payload=b""):
    return sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + bytes(8) + bytes([0x50, 0x10]) + \
        bytes(6) + payload


def ip4(a, b, c, d):
    return bytes([a, b, c, d])


def hand_rows():
    """One frame a branch of the programs: [(name, frame bytes)]."""
    A, B = ip4(10, 0, 0, 1), ip4(10, 0, 0, 2)
    A6 = bytes(range(1, 17))
    B6 = bytes(range(101, 117))
    u = udp(4000, 53, b"x" * 4)
    Q, AD = ETH_P_8021Q, ETH_P_8021AD
    rows = [
        ("v4_udp", eth(ETH_P_IP, ipv4(A, B, 17, u))),
        ("v4_udp_tag", eth(ETH_P_IP, ipv4(A, B, 17, u), tags=(Q,))),
        ("v4_udp_qinq", eth(ETH_P_IP, ipv4(A, B, 17, u), tags=(AD, Q))),
        ("v4_udp_three_tags", eth(ETH_P_IP, ipv4(A, B, 17, u), tags=(AD, Q, Q))),
        ("ethertype_05ff", eth(0x05ff, ipv4(A, B, 17, u))),
        ("short_13", eth(ETH_P_IP, b"")[:13]),
        ("tag_cut_17", eth(ETH_P_IP, ipv4(A, B, 17, u), tags=(Q,))[:17]),
        ("second_tag_cut_21", eth(ETH_P_IP, ipv4(A, B, 17, u), tags=(AD, Q))[:21]),
        ("v4_cut_l3_19", eth(ETH_P_IP, ipv4(A, B, 17, u))[:14 + 19]),
        ("v4_exact_l3_20", eth(ETH_P_IP, ipv4(A, B, 17, u))[:14 + 20]),
        ("v6_qinq_61", eth(ETH_P_IPV6, ipv6(A6, B6, 17, u), tags=(AD, Q))[:61]),
        ("v6_qinq_62", eth(ETH_P_IPV6, ipv6(A6, B6, 17, u), tags=(AD, Q))[:62]),
        ("v6_udp", eth(ETH_P_IPV6, ipv6(A6, B6, 17, u))),
        ("v6_tcp_tag", eth(ETH_P_IPV6, ipv6(A6, B6, 6, tcp(40000, 443)), tags=(Q,))),
        ("v6_tcp_qinq", eth(ETH_P_IPV6, ipv6(A6, B6, 6, tcp(40001, 8443)), tags=(AD, Q))),
        ("v6_udp_qinq", eth(ETH_P_IPV6, ipv6(A6, B6, 17, udp(40002, 4789)), tags=(Q, Q))),
        ("arp", eth(0x0806, bytes(28))),
        ("v4_ihl6_udp", eth(ETH_P_IP, ipv4(A, B, 17, udp(7, 9) + udp(1234, 5678), ihl=6))),
        ("udp_7_bytes", eth(ETH_P_IP, ipv4(A, B, 17, udp(4000, 53)))[:14 + 20 + 7]),
        ("udp_8_bytes", eth(ETH_P_IP, ipv4(A, B, 17, udp(4000, 53)))[:14 + 20 + 8]),
        ("tcp_19_bytes", eth(ETH_P_IP, ipv4(A, B, 6, tcp(4001, 80)))[:14 + 20 + 19]),
        ("tcp_20_bytes", eth(ETH_P_IP, ipv4(A, B, 6, tcp(4001, 80)))[:14 + 20 + 20]),
        ("icmp", eth(ETH_P_IP, ipv4(A, B, 1, bytes(16)))),
        ("v4_udp_swapped", eth(ETH_P_IP, ipv4(B, A, 17, udp(53, 4000, b"x" * 4)))),
        ("v6_udp_swapped", eth(ETH_P_IPV6, ipv6(B6, A6, 17, udp(53, 4000, b"x" * 4)))),
    ]
    return rows

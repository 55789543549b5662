"""The forwarded egress call (xfg_forward_egress) as a numpy/Python model,
written from xdp-forward's text and held equal to the program itself, compiled
for the host, by tests/test_forward_reference.py: xdp_fwd_flags() of
xdp-forward/xdp_forward.bpf.c (:32-127, ip_decrease_ttl :23-30) over headers/xdp/parsing_helpers.h's
parse_ethhdr (:100-134, VLAN_MAX_DEPTH 4, :80) and parse_iphdr (:201-233),
with bpf_fib_lookup (a kernel helper) replaced by a longest-prefix match over a
route list.  The match here is brute force -- lpm() tries every route;
lpm_many() tries every length, longest first, every address at once -- and
shares nothing with the C builder's DIR-24-8 tables.
"""
import numpy as np

PASS = 2
QUEUE_NONE = 0xff
ADDR48 = (1 << 48) - 1
(OK, NOT_IP, BAD_HDR, TTL, V6, NO_ROUTE, NH_RET, FRAG, NO_PORT) = range(9)
REASONS = 9
REASON_NAMES = ["OK", "NOT_IP", "BAD_HDR", "TTL", "V6", "NO_ROUTE", "NH_RET", "FRAG", "NO_PORT"]
ETH_P_IP, ETH_P_IPV6, ETH_P_8021Q, ETH_P_8021AD, ETH_P_ARP = 0x0800, 0x86DD, 0x8100, 0x88A8, 0x0806
VLAN_MAX_DEPTH = 4                      # parsing_helpers.h:80


# ---- the FIB
def mask_of(length):
    return (0xffffffff << (32 - length)) & 0xffffffff if length else 0


def lpm(routes, dst):
    """routes: (prefix, len, nexthop) triples, prefix in host order.  The next
    hop of the longest route that covers dst, or None: every route is tried."""
    best = None
    for prefix, length, nh in routes:
        if (dst & mask_of(length)) == prefix and (best is None or length > best[0]):
            best = (length, nh)
    return None if best is None else best[1]


def lpm_many(routes, dsts):
    """lpm() for an array of addresses: -1 where no route covers one.  Length
    by length, longest first: an address not yet matched is looked for, masked,
    among that length's prefixes."""
    dsts = np.asarray(dsts, np.uint64)
    out = np.full(len(dsts), -1, np.int64)
    r = np.asarray(routes, np.int64).reshape(-1, 3)
    for length in range(32, -1, -1):
        sel = r[r[:, 1] == length]
        if not len(sel):
            continue
        order = np.argsort(sel[:, 0], kind="stable")
        pre, nh = sel[order, 0].astype(np.uint64), sel[order, 2]
        todo = np.flatnonzero(out < 0)
        key = dsts[todo] & np.uint64(mask_of(length))
        at = np.minimum(np.searchsorted(pre, key), len(pre) - 1)
        hit = pre[at] == key
        out[todo[hit]] = nh[at[hit]]
    return out


# ---- one frame
def parse_ethhdr(f):
    """parsing_helpers.h:100-134: (ethertype, l3) or None if the Ethernet
    header does not fit (:108-109).  A tag that does not fit ends the loop with
    the VLAN ethertype (:123-124), and so does a fifth tag (:119)."""
    if len(f) < 14:
        return None
    ty, at = int.from_bytes(f[12:14], "big"), 14
    for _ in range(VLAN_MAX_DEPTH):
        if ty not in (ETH_P_8021Q, ETH_P_8021AD):     # :120-121
            break
        if at + 4 > len(f):                           # :123-124
            break
        ty = int.from_bytes(f[at + 2:at + 4], "big")  # :126
        at += 4
    return ty, at


def decrease_ttl(check_le):
    """ip_decrease_ttl's checksum step (:25-28) on the field as a little-endian
    16-bit load of its bytes sees it; htons(0x0100) is then 0x0001."""
    c = check_le + 0x0001
    return (c + (1 if c >= 0xFFFF else 0)) & 0xffff


def forward_frame(f, lookup, nexthops, ports):
    """xdp_fwd_flags() over frame bytes f.  lookup(dst) -> next hop index or
    None; nexthops: (ifindex, mtu, ret, dmac, smac) tuples; ports: the ifindex
    list of xdp_tx_ports.  Returns (reason, queue or None, the frame after)."""
    p = parse_ethhdr(f)
    if p is None:
        return NOT_IP, None, f                         # xdp_forward.bpf.c:45, :81-83
    ty, l3 = p
    if ty == ETH_P_IP:                                 # :46
        if l3 + 20 > len(f):                           # parsing_helpers.h:209-210
            return BAD_HDR, None, f
        if l3 + 4 * (f[l3] & 0xf) > len(f):            # :212-216; no ihl >= 5 check
            return BAD_HDR, None, f
        if f[l3 + 8] <= 1:                             # xdp_forward.bpf.c:51-52
            return TTL, None, f
    elif ty == ETH_P_IPV6:                             # :62: no IPv6 table, :126
        return V6, None, f
    else:
        return NOT_IP, None, f                         # :81-83
    dst = int.from_bytes(f[l3 + 16:l3 + 20], "big")    # :61
    nh = lookup(dst)
    if nh is None:
        return NO_ROUTE, None, f                       # :126
    ifindex, mtu, ret, dmac, smac = nexthops[nh]
    if ret:
        return NH_RET, None, f                         # :126
    if mtu and int.from_bytes(f[l3 + 2:l3 + 4], "big") > mtu:   # :59
        return FRAG, None, f
    if ifindex not in ports:                           # :113-114
        return NO_PORT, None, f
    g = bytearray(f)
    g[l3 + 10:l3 + 12] = decrease_ttl(int.from_bytes(f[l3 + 10:l3 + 12], "little")).to_bytes(2, "little")
    g[l3 + 8] -= 1                                     # :29
    g[0:6], g[6:12] = bytes(dmac), bytes(smac)         # :121-122
    return OK, list(ports).index(ifindex), bytes(g)


# ---- a batch
def forward_model(pool, fid, addr, lens, v, routes, nexthops, ports):
    """Records i name pool frame fid[i] (bytes [0, lens[i]) at addr[i]), with
    verdicts v.  Returns (tx, fill, counts, queue_of, reason_of, after): tx[q]
    the (k, 2) u64 TX records of queue q (q == len(ports): the stack ring), fill
    the other records' chunk addresses, counts the len(ports) + 2 + REASONS
    counts, and after[i] record i's frame bytes when the call has run."""
    n, P = len(v), len(ports)
    fid = np.asarray(fid, np.int64)
    passed = np.asarray(v) == PASS
    used = np.unique(fid[passed]) if n else np.zeros(0, np.int64)
    memo = {}

    def lookup(dst):
        if dst not in memo:
            memo[dst] = lpm(routes, dst)
        return memo[dst]

    per = {int(k): forward_frame(pool[k], lookup, nexthops, ports) for k in used}
    queue_of = np.full(n, QUEUE_NONE, np.uint8)
    reason_of = np.full(n, QUEUE_NONE, np.uint8)
    after = [pool[k] for k in fid]
    for i in np.flatnonzero(passed):
        r, q, g = per[int(fid[i])]
        reason_of[i] = r
        queue_of[i] = P if q is None else q
        after[i] = g
    addr = np.asarray(addr, np.uint64)
    lens = np.asarray(lens)
    tx = []
    for q in range(P + 1):
        m = queue_of == q
        rec = np.empty((int(m.sum()), 2), np.uint64)
        rec[:, 0] = addr[m]
        rec[:, 1] = lens[m].astype(np.uint64)          # options 0
        tx.append(rec)
    other = ~passed
    fill = addr[other] & np.uint64(ADDR48)
    counts = np.array([len(t) for t in tx] + [int(other.sum())] +
                      [int((reason_of == r).sum()) for r in range(REASONS)], np.uint64)
    return tx, fill, counts, queue_of, reason_of, after


# ---- frames for the tests
def eth(ethertype, payload, tags=(), dst=b"\x02\x00\x00\x00\x00\x01", src=b"\x02\x00\x00\x00\x00\x02"):
    """An Ethernet frame: @tags the TPIDs of its VLAN tags, outermost first."""
    h = dst + src
    for k, tpid in enumerate(tags):
        h += tpid.to_bytes(2, "big") + (100 + k).to_bytes(2, "big")
    return h + ethertype.to_bytes(2, "big") + payload


def csum16(b):
    """The ones' complement sum of the 16-bit big-endian words of b."""
    s = sum(int.from_bytes(b[i:i + 2], "big") for i in range(0, len(b), 2))
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return s


def ipv4(daddr, saddr=b"\xc0\x00\x02\x01", ttl=64, proto=17, payload=b"", ihl=5, tot_len=None,
         check=None, tos=0, ident=0):
    """An IPv4 header of max(ihl, 5) * 4 bytes (options zero) that claims ihl,
    and the payload; check None: the valid checksum."""
    room = 4 * max(ihl, 5)
    tl = room + len(payload) if tot_len is None else tot_len
    h = bytearray(bytes([0x40 | ihl, tos]) + tl.to_bytes(2, "big") + ident.to_bytes(2, "big") +
                  bytes(2) + bytes([ttl, proto]) + bytes(2) + saddr + daddr + bytes(room - 20))
    c = (~csum16(bytes(h[:4 * ihl] if ihl >= 5 else h[:20])) & 0xffff) if check is None else check
    h[10:12] = c.to_bytes(2, "big")
    return bytes(h) + payload


def ip_bytes(a):
    return int(a).to_bytes(4, "big")

"""The corpus of the forwarded egress GPU tests (tests/test_gpu_forward.py): a
FIB, a port table and a pool of distinct frames for a number of ports.  Built
without a GPU, so tests/test_forward_model.py asserts the corpus conditions on
the model alone: every reason occurs, every port and the stack ring receive
records, and forwarded frames resolve both in the first table and through a
second-level group."""
import functools

import numpy as np

import fwdmodel as M

TILE = 2048
POOL = 3 * TILE + 5                     # the largest batch: every record its own frame
N3 = POOL                               # a batch of three tiles and five records
IF_ABSENT = 9999                        # an ifindex no port table has
OTHERS = np.array([0, 1, 3, 4, 255], np.uint8)


def verdicts_of(n, pattern, seed=0):
    """n verdict bytes: about 70% PASS among the other values, all PASS, or none."""
    rng = np.random.default_rng(8 * n + seed)
    v = OTHERS[rng.integers(0, len(OTHERS), n)]
    if pattern == "random":
        v[rng.random(n) < 0.7] = M.PASS
    elif pattern == "all_pass":
        v[:] = M.PASS
    return v


def ifindexes(nports):
    return [100 + 7 * q for q in range(nports)]


def mac(k, side):
    return bytes([0x02, side, 0, 0, k >> 8, k & 0xff])


@functools.lru_cache(maxsize=None)
def fib_of(nports):
    """(routes, nexthops): two good next hops a port, then a blackhole (ret
    != 0), one with a small mtu and one whose ifindex no port has; fixed nested
    routes over 10.1.2.200, random routes of lengths 8..32 inside 20.0.0.0/8
    (no default route: 11.0.0.0/8 has none at all)."""
    rng = np.random.default_rng(1000 + nports)
    ifx = ifindexes(nports)
    nexthops = [(ifx[k % nports], 0 if k % 3 else 1500, 0, mac(k, 1), mac(k, 2)) for k in range(2 * nports)]
    good = len(nexthops)
    nexthops += [(ifx[0], 0, 3, mac(900, 1), mac(900, 2)),            # NH_RET
                 (ifx[-1], 100, 0, mac(901, 1), mac(901, 2)),         # FRAG above 100
                 (IF_ABSENT, 0, 0, mac(902, 1), mac(902, 2))]         # NO_PORT
    routes = {(0x0a000000, 8): 0, (0x0a010000, 16): 1 % good, (0x0a010200, 24): 2 % good,
              (0x0a010280, 25): 3 % good, (0x0a0102c8, 32): 4 % good,
              (0xc0a80000, 16): good, (0xac100000, 12): good + 1, (0x0a090000, 16): good + 2}
    for j in range(4 * nports + 60):
        length = int(rng.integers(8, 33))
        prefix = (0x14000000 | int(rng.integers(1 << 24))) & M.mask_of(length)
        routes.setdefault((prefix, length), j % good)
    return tuple((p, l, nh) for (p, l), nh in routes.items()), tuple(nexthops)


def inside(rng, route):
    prefix, length, _ = route
    return prefix | (int(rng.integers(1 << 32)) & ~M.mask_of(length) & 0xffffffff)


TAGS = [(), (M.ETH_P_8021Q,), (M.ETH_P_8021AD, M.ETH_P_8021Q), (M.ETH_P_8021AD,) * 2 + (M.ETH_P_8021Q,),
        (M.ETH_P_8021Q,) * 4]


def frame(rng, k, routes, n_routed):
    """Pool frame k: most go through the lookup, the others by turns through
    every other branch."""
    r = lambda m: bytes(rng.integers(0, 256, m, dtype=np.uint8))     # noqa: E731
    tags = TAGS[k % 5]
    src = r(4)
    payload = r(int(rng.integers(0, 13)))
    ttl = int(rng.integers(2, 256))
    kind = k % 16
    if kind < 8:      # routed: a random route's address (good and special next hops alike)
        dst = inside(rng, routes[int(rng.integers(n_routed))])
        ihl = [5, 5, 5, 6, 15, 0, 3, 5][(k // 16) % 8] if len(tags) < 2 else 5
        check = None if k % 3 else int(rng.integers(0, 65536))
        return M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(dst), src, ttl, payload=payload, ihl=ihl, check=check,
                                        tos=k & 0xff, ident=k & 0xffff), tags)
    if kind == 8:     # the special next hops: NH_RET, FRAG (tot_len above and below 100), NO_PORT
        which = (k // 16) % 4
        dst = [0xc0a80000, 0xac100000, 0xac100000, 0x0a090000][which] | int(rng.integers(1 << 16))
        tot = [None, 101 + int(rng.integers(60000)), 100, None][which]
        return M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(dst), src, ttl, payload=payload, tot_len=tot), tags)
    if kind == 9:     # no route
        return M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(0x0b000000 | int(rng.integers(1 << 24))), src, ttl,
                                        payload=payload), tags)
    if kind == 10:    # ttl 0 and 1
        return M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(0x0a010203), src, (k // 16) % 2, payload=payload), tags)
    if kind == 11:    # IPv6
        return M.eth(M.ETH_P_IPV6, bytes([0x60, 0, 0, 0, 0, 8, 17, 64]) + r(32) + r(8), tags)
    if kind == 12:    # a header cut short, or an ihl that does not fit
        f = M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(0x0a010203), src, ttl, ihl=[5, 9, 15][(k // 16) % 3]), tags)
        return f[:len(f) - 1 - int(rng.integers(0, 19))] + b""
    if kind == 13:    # not IP: ARP, a fifth tag, an old-style length
        ty = [M.ETH_P_ARP, M.ETH_P_8021Q, 0x0040][(k // 16) % 3]
        return M.eth(ty, r(28), tags if ty != M.ETH_P_8021Q else TAGS[4])
    if kind == 14:    # a tag cut: the frame ends 0..3 bytes into its last tag
        f = M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(0x0a010203), src, ttl), TAGS[1 + k % 4])
        return f[:14 + 4 * (k % 4) + (k // 16) % 4]
    return r((k // 16) % 14)        # shorter than an Ethernet header


@functools.lru_cache(maxsize=None)
def pool_of(nports):
    """POOL frames of at most 96 bytes, a frame a record and a chunk of its
    own, so no frame is rewritten twice (some of the short ones, which are
    never forwarded, have equal bytes)."""
    rng = np.random.default_rng(2000 + nports)
    routes, _ = fib_of(nports)
    pool = [frame(rng, k, routes, len(routes)) for k in range(POOL)]
    assert max(map(len, pool)) <= 96
    return tuple(pool)


@functools.lru_cache(maxsize=None)
def one_flow_pool():
    """3 * TILE + 5 frames of one destination behind 10.1.2.128/25: every
    record takes the same port, through a second-level group."""
    rng = np.random.default_rng(77)
    return tuple(M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(0x0a010281), bytes(rng.integers(0, 256, 4, dtype=np.uint8)),
                                          64, ident=k & 0xffff)) for k in range(POOL))

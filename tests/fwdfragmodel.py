"""A plain-Python/numpy model of xfg_forward_frags_egress (include/xdpfilter_gpu.h,
"Forwarded egress of multi-buffer packets"), put together from two models that
are tested on their own: steerfragmodel.packets() -- how records form packets
-- and fwdmodel.forward_frame() -- xdp-forward's program on one buffer, held
equal to the program itself by test_forward_reference.py.  An XDP program sees
only a packet's first buffer, so the head's frame decides the packet.

Behind the model: the inputs of the GPU cases (tests/test_gpu_forward_frags.py),
built without a GPU so that tests/test_forward_frags_model.py can assert the
condition every case is named for.
"""
import functools

import numpy as np

import fwdcorpus as K
import fwdmodel as M
import steerfragmodel as F

PASS, NONE, CONTD = M.PASS, F.VERDICT_NONE, F.CONTD
QUEUE_NONE, ADDR48, REASONS = M.QUEUE_NONE, M.ADDR48, M.REASONS
T = K.TILE
CHUNK = 128             # a frame of at most 96 bytes at headroom 0 / 16 / 32
OTHERS = np.array([0, 1, 3, 4], np.uint8)


# ---- the model
def forward_frags_model(pool, fid, addr, lens, opts, v, routes, nexthops, ports):
    """Record i's chunk holds pool frame fid[i] (bytes [0, lens[i]) at addr[i]).
    Returns (tx, fill, counts, queue_of, reason_of, ok, per): tx[q] the (k, 2)
    u64 TX records of queue q in order (q == len(ports): the stack ring), fill
    the chunk addresses of the fill side in order, counts the len(ports) + 2 +
    REASONS counts, ok[i] true for the heads that are rewritten and per[k] =
    (reason, queue or None, frame after) of every pool frame that is a PASS
    head -- the only frames that are looked at."""
    n, P = len(v), len(ports)
    v = np.asarray(v)
    opts = np.asarray(opts, np.uint32)
    fid = np.asarray(fid, np.int64)
    live, head, head_of = F.packets(v, opts)
    pass_heads = np.flatnonzero(head & (v == PASS))
    memo = {}

    def lookup(dst):
        if dst not in memo:
            memo[dst] = M.lpm(routes, dst)
        return memo[dst]

    per = {int(k): M.forward_frame(pool[k], lookup, nexthops, ports) for k in np.unique(fid[pass_heads])}
    head_q = np.full(n, QUEUE_NONE, np.uint8)
    head_r = np.full(n, QUEUE_NONE, np.uint8)
    if len(pass_heads):
        # PASS head, XFG_FWD_OK: port q; PASS head, any other reason: the stack ring
        head_q[pass_heads] = [P if per[int(k)][1] is None else per[int(k)][1] for k in fid[pass_heads]]
        head_r[pass_heads] = [per[int(k)][0] for k in fid[pass_heads]]
    # the packet's queue and reason for every live record of a PASS packet
    at = np.maximum(head_of, 0)
    queue_of = np.where(live, head_q[at], QUEUE_NONE).astype(np.uint8)
    reason_of = np.where(live, head_r[at], QUEUE_NONE).astype(np.uint8)
    addr = np.asarray(addr, np.uint64)
    word1 = np.asarray(lens).astype(np.uint64) | ((opts & CONTD).astype(np.uint64) << np.uint64(32))
    tx = []
    for q in range(P + 1):
        m = queue_of == q
        r = np.empty((int(m.sum()), 2), np.uint64)
        r[:, 0], r[:, 1] = addr[m], word1[m]
        tx.append(r)
    other = live & (queue_of == QUEUE_NONE)
    fill = addr[other] & np.uint64(ADDR48)
    # the reasons count PASS packets: only heads are parsed
    counts = np.array([len(r) for r in tx] + [int(other.sum())] +
                      np.bincount(head_r[pass_heads], minlength=REASONS).tolist(), np.uint64)
    ok = np.zeros(n, bool)
    ok[pass_heads] = head_r[pass_heads] == M.OK
    return tx, fill, counts, queue_of, reason_of, ok, per


def walk(frames, addr, lens, opts, v, routes, nexthops, ports):
    """The same, record by record, as a consumer loop with one packet's state
    would do it.  frames[i]: record i's bytes.  Returns (tx, fill, counts,
    queue_of, reason_of, after): after[i] record i's bytes when it has run."""
    P = len(ports)
    tx = [[] for _ in range(P + 1)]
    fill, queue_of, reason_of, after = [], [], [], list(frames)
    reasons = [0] * REASONS
    cur = None          # the open packet's (queue, reason); None: no packet open
    for i in range(len(v)):
        if v[i] == NONE:
            queue_of.append(QUEUE_NONE)
            reason_of.append(QUEUE_NONE)
            cur = None
            continue
        if cur is None:             # a head
            cur = (QUEUE_NONE, QUEUE_NONE)
            if v[i] == PASS:
                r, q, g = M.forward_frame(frames[i], lambda d: M.lpm(routes, d), nexthops, ports)
                cur = (P if q is None else q, r)
                reasons[r] += 1
                after[i] = g
        if cur[0] == QUEUE_NONE:
            fill.append(int(addr[i]) & ADDR48)
        else:
            tx[cur[0]].append((int(addr[i]), int(lens[i]) | (int(opts[i]) & CONTD) << 32))
        queue_of.append(cur[0])
        reason_of.append(cur[1])
        if not int(opts[i]) & CONTD:
            cur = None
    return tx, fill, [len(t) for t in tx] + [len(fill)] + reasons, queue_of, reason_of, after


# ---- the frames of the GPU cases
NSPECIAL = 80


def routable(ttl, k):
    """A frame 10.1.2.3 forwards (10.1.2.0/24: a good next hop without an mtu)
    but for its TTL."""
    return M.eth(M.ETH_P_IP, M.ipv4(M.ip_bytes(0x0a010203), b"\xc0\x00\x02\x07", ttl, payload=b"hazard", ident=k))


@functools.lru_cache(maxsize=None)
def pool_of(nports):
    """fwdcorpus.pool_of(nports), and behind it NSPECIAL frames with TTL 2 (at
    TTL2), NSPECIAL with TTL 1 (at TTL1): otherwise routable and equal."""
    return K.pool_of(nports) + tuple(routable(2, k) for k in range(NSPECIAL)) + \
        tuple(routable(1, k) for k in range(NSPECIAL))


TTL2 = K.POOL
TTL1 = K.POOL + NSPECIAL


@functools.lru_cache(maxsize=None)
def pool_matrix(nports):
    pool = pool_of(nports)
    m = np.zeros((len(pool), 96), np.uint8)
    for k, f in enumerate(pool):
        m[k, :len(f)] = np.frombuffer(f, np.uint8)
    lens = np.array([len(f) for f in pool], np.uint32)
    m.setflags(write=False)
    lens.setflags(write=False)
    return m, lens


def put(umem, chunk, room, rows, lens):
    """rows[j, :lens[j]] to chunk[j] of the UMEM at headroom room[j]."""
    u = umem.reshape(-1, CHUNK)
    cols = np.arange(96)
    for h in (0, 16, 32):
        s = np.flatnonzero(room == h)
        keep = cols[None, :] < lens[s][:, None]
        part = u[chunk[s], h:h + 96]
        part[keep] = rows[s][keep]
        u[chunk[s], h:h + 96] = part


def umem_of_records(nports, fid, seed=3):
    """A UMEM of random bytes with a chunk of its own for every record, in
    permuted order, record i's chunk holding pool frame fid[i] at headroom 0 /
    16 / 32, every third address in the unaligned-chunk form.  Returns (umem,
    addr, lens, chunk, room)."""
    pm, plens = pool_matrix(nports)
    n = len(fid)
    rng = np.random.default_rng(seed)
    nchunks = n + 7
    umem = rng.integers(0, 256, nchunks * CHUNK, dtype=np.uint8)
    chunk = rng.permutation(nchunks)[:n]
    i = np.arange(n)
    room = 16 * (i % 3)
    lens = plens[fid]
    put(umem, chunk, room, pm[fid], lens)
    base = chunk.astype(np.uint64) * np.uint64(CHUNK)
    h = room.astype(np.uint64)
    addr = np.where(i % 3 == 2, base | (h << np.uint64(48)), base + h).astype(np.uint64)
    return umem, addr, lens, chunk, room


def umem_after(umem, fid, chunk, room, ok, per):
    """The UMEM when the call has run: the rewritten heads' frames."""
    want = umem.copy()
    rows = np.flatnonzero(ok)
    if len(rows):
        after = np.zeros((len(rows), 96), np.uint8)
        lens = np.zeros(len(rows), np.uint32)
        for j, k in enumerate(fid[rows]):
            g = per[int(k)][2]
            after[j, :len(g)] = np.frombuffer(g, np.uint8)
            lens[j] = len(g)
        put(want, chunk[rows], room[rows], after, lens)
    return want


# ---- the records of the GPU cases
def plens_of(n, shape, seed=0):
    """Packet lengths that cover n records."""
    if shape == "single":
        return np.ones(n, np.int64)
    if shape == "three":
        return np.full(n // 3 + 1, 3, np.int64)
    return np.random.default_rng(1000 + n + seed).integers(1, 19, n)


def verdicts(n, seed=0, none=0.0):
    """A byte a record, drawn record by record (so a continuation's byte
    differs from its head's more often than not): 60 % PASS."""
    rng = np.random.default_rng(8 * n + seed)
    v = OTHERS[rng.integers(0, len(OTHERS), n)]
    v[rng.random(n) < 0.6] = PASS
    v[rng.random(n) < none] = NONE
    return v


def option_words(plens, n):
    """XDP_PKT_CONTD by the packet lengths, and on every fifth record a bit a
    TX record must not carry."""
    return F.opts_of_packet_lengths(plens, n) | np.where(np.arange(n) % 5 == 4, 1 << 16, 0).astype(np.uint32)


def fids(n, seed=0):
    """A corpus frame a record: continuation chunks hold whole frames of other
    flows, most of them routable."""
    return np.random.default_rng(100 + n + seed).integers(0, K.POOL, n)


N3 = 3 * T + 7
SIZES = [T - 1, T, T + 1, N3]
PORTS = [1, 8, 63]
SHAPES = ["single", "three", "random"]
PLACEMENTS = {
    # a head on a tile's first record; a packet ending on a tile's last record
    "tile_edges": ([T - 4, 4, 3], N3),
    # a head on a tile's last record, its continuations in the next tile
    "head_on_tile_last": ([T - 1, 4], N3),
    # heads in a wave's last lane, their continuations in the next wave (or pass)
    "wave_last_lane": ([63] + [64] * 40, N3),
    # 70 records straddling a tile boundary, the head 67 before it
    "straddle_70": ([T - 67, 70], N3),
    # 2T + 3 records: tile 1 holds no head and hands on what it is handed
    "two_tiles_and_3": ([5, 2 * T + 3], N3 + 93),
    # a straddle across the RX ring's wrap (rot 1: the RX ring wraps mid-batch)
    "wrap": ([1500, 600], N3),
}


def placement(name, head, ttl=None):
    """(fid, opts, v, long_head): the placement's long packet with a PASS or
    other head; @ttl 2 or 1: its head is the otherwise routable frame."""
    first, n = PLACEMENTS[name]
    opts = option_words(np.concatenate([first, plens_of(n, "three")]), n)
    v = verdicts(n, 3)
    fid = fids(n, 3)
    long_head = int(np.sum(first[:-1]))
    v[long_head] = PASS if head == "pass" else 1
    if ttl:
        fid[long_head] = TTL2 if ttl == 2 else TTL1
    return fid, opts, v, long_head


HAZARD_TILES = 64


def hazard(ttl):
    """HAZARD_TILES tiles of three-record packets in which every tile boundary
    b is straddled by a five-record PASS packet, records b - 2 .. b + 2, whose
    head is routable but for its TTL @ttl.  Returns (fid, opts, v, heads)."""
    n = HAZARD_TILES * T
    opts = option_words(plens_of(n, "three"), n)
    v = verdicts(n, 20 + ttl)
    fid = fids(n, 20 + ttl)
    b = np.arange(1, HAZARD_TILES) * T
    for d in (-3, 2):
        opts[b + d] &= ~np.uint32(CONTD)
    for d in (-2, -1, 0, 1):
        opts[b + d] |= CONTD
        v[b + d] = OTHERS[(b + d) % 4]          # not VERDICT_NONE: the packet is whole
    v[b - 3] = 1                                # (live: record b - 2 is a head by the end of packet before it)
    heads = b - 2
    v[heads] = PASS
    fid[heads] = (TTL2 if ttl == 2 else TTL1) + np.arange(len(b))
    return fid, opts, v, heads


NONE_RUNS = {"middle": [(700, 790), (T + 100, T + 101)], "tile_last": [(T - 1, T), (2 * T - 9, 2 * T)],
             "tile_first": [(T, T + 1), (2 * T, 2 * T + 70)], "all": [(0, N3)]}


def none_runs(where):
    n = N3
    opts = option_words(plens_of(n, "random", 4), n)
    v = verdicts(n, 4)
    for a, b in NONE_RUNS[where]:
        v[a:b] = NONE
    return fids(n, 4), opts, v


def every_reason():
    """Three tiles of three-record PASS packets: every reason on a packet of
    several records."""
    n = N3
    opts = option_words(plens_of(n, "three"), n)
    v = verdicts(n, 6)
    v[::3] = PASS
    return fids(n, 6), opts, v

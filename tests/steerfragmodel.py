"""A plain-Python/numpy model of xfg_steer_frags_egress (include/xdpfilter_gpu.h,
"Steered egress of multi-buffer packets"): how records form packets, the queue
a packet takes from its head, the K-way order-preserving partition of the live
records and the counts.

The head's queue is steermodel.queue_of_frame() -- the reference's parse_eth,
cpumap_l4_hash, cpumap_l4_sport and cpumap_l4_dport (xdp-bench/
xdp_redirect_cpumap.bpf.c:53-96, 506-653) on the head buffer, which is all an
XDP program sees of a multi-buffer packet; test_steer_reference.py holds that
function equal to those programs.  Every other rule cites the header comment
("H:" below, by its sentence).
"""
import numpy as np

import steermodel as M

PASS = M.PASS
VERDICT_NONE = 0xff     # XFG_VERDICT_NONE
CONTD = 1               # XFG_XDP_PKT_CONTD, headers/linux/if_xdp.h:123
QUEUE_NONE = M.QUEUE_NONE
ADDR48 = M.ADDR48


def packets(v, opts):
    """(live, head, head_of): head_of[i] is the index of record i's head, -1
    for a record that is not live.
    H: live[i] = v[i] != XFG_VERDICT_NONE; eop[i] = !(o[i] & XFG_XDP_PKT_CONTD);
    head[i] = live[i] && (i == 0 || !live[i-1] || eop[i-1]); a live record
    belongs to the nearest head at or before it."""
    v = np.asarray(v)
    opts = np.asarray(opts)
    n = len(v)
    live = v != VERDICT_NONE
    eop = (opts & CONTD) == 0
    head = live.copy()
    if n > 1:
        head[1:] &= ~live[:-1] | eop[:-1]
    at = np.where(head, np.arange(n), -1)
    head_of = np.maximum.accumulate(at) if n else at
    head_of = np.where(live, head_of, -1)
    return live, head, head_of


def steer_frags_model(frames, addr, lens, opts, v, nqueues, mode=M.L4_HASH, avail=None, skip_queue=0,
                      fid=None):
    """frames[i]: record i's bytes [0, lens[i]) -- or, with @fid, frames a pool
    and frames[fid[i]] record i's.  Only the frames of PASS heads are looked at
    (H: "no UMEM byte of a record that is not a PASS head is read").
    Returns (tx, fill, counts, queue_of): tx[q] the (k, 2) u64 TX records of
    queue q in order ({addr, len | options << 32}), fill the chunk addresses of
    the fill side in order, counts the nqueues + 2 counts, queue_of the byte a
    record."""
    n = len(v)
    v = np.asarray(v)
    opts = np.asarray(opts, np.uint32)
    avail = list(range(nqueues)) if avail is None else list(avail)
    live, head, head_of = packets(v, opts)
    # H: "A packet whose head byte is XFG_XDP_PASS takes the queue
    # xfg_steer_egress would give the head record's frame"; "a packet whose head
    # byte is anything else hands every live record's chunk to the fill ring"
    head_q = np.full(n, QUEUE_NONE, np.uint8)
    pass_heads = np.flatnonzero(head & (v == PASS))
    if fid is None:
        refused = 0
        for h in pass_heads:
            q, r = M.queue_of_frame(frames[h], mode, avail, skip_queue)
            head_q[h] = q
            refused += r             # H: counts[nqueues + 1] "per packet"
    else:                            # (each pool frame parsed once)
        fid = np.asarray(fid, np.int64)
        per = [M.queue_of_frame(f, mode, avail, skip_queue) for f in frames]
        pq = np.array([q for q, _ in per], np.uint8)
        pr = np.array([r for _, r in per], bool)
        head_q[pass_heads] = pq[fid[pass_heads]]
        refused = int(pr[fid[pass_heads]].sum())
    # H: queue_of[i] "the packet's queue for every live record of a PASS
    # packet, XFG_QUEUE_NONE for every other record, those that are not live
    # included"
    queue_of = np.where(live, head_q[np.maximum(head_of, 0)], QUEUE_NONE).astype(np.uint8)
    addr = np.asarray(addr, np.uint64)
    lens = np.asarray(lens)
    # H: "addr and len as received, options = the RX record's options &
    # XFG_XDP_PKT_CONTD"
    word1 = lens.astype(np.uint64) | ((opts & CONTD).astype(np.uint64) << np.uint64(32))
    tx = []
    for q in range(nqueues):
        m = queue_of == q
        r = np.empty((int(m.sum()), 2), np.uint64)
        r[:, 0] = addr[m]
        r[:, 1] = word1[m]
        tx.append(r)
    # H: "The j-th live record on the fill side"; "A record that is not live
    # produces nothing"
    other = live & (queue_of == QUEUE_NONE)
    fill = addr[other] & np.uint64(ADDR48)
    counts = np.array([len(r) for r in tx] + [int(other.sum()), refused], np.uint64)
    return tx, fill, counts, queue_of


def walk(frames, addr, lens, opts, v, nqueues, mode=M.L4_HASH, avail=None, skip_queue=0):
    """The same, record by record, as a consumer loop with one packet's state
    would do it."""
    avail = list(range(nqueues)) if avail is None else list(avail)
    tx = [[] for _ in range(nqueues)]
    fill, queue_of, refused = [], [], 0
    cur = None          # the open packet's queue (QUEUE_NONE: fill side), None: no packet open
    for i in range(len(v)):
        if v[i] == VERDICT_NONE:
            queue_of.append(QUEUE_NONE)
            cur = None
            continue
        if cur is None:             # a head
            cur = QUEUE_NONE
            if v[i] == PASS:
                cur, r = M.queue_of_frame(frames[i], mode, avail, skip_queue)
                refused += r
        if cur == QUEUE_NONE:
            fill.append(int(addr[i]) & ADDR48)
        else:
            tx[cur].append((int(addr[i]), int(lens[i]) | (int(opts[i]) & CONTD) << 32))
        queue_of.append(cur)
        if not int(opts[i]) & CONTD:
            cur = None
    return tx, fill, [len(t) for t in tx] + [len(fill), refused], queue_of


def opts_of_packet_lengths(plens, n):
    """Option words of @n records cut into packets of plens[0], plens[1], ...
    records (the last one cut short, and then left open, if they pass n)."""
    o = np.full(n, CONTD, np.uint32)
    ends = np.cumsum(np.asarray(plens, np.int64)) - 1
    o[ends[ends < n]] = 0
    return o

"""What xfg_classify_socks_frags and xfg_socks_frags_egress compute
(include/xdpfilter_gpu.h), as numpy over the flat arrays -- fragmodel.frag_model
a socket, sockmodel.sock_model over the live records -- and the same as a plain
record-by-record walk, l2fwd() on every socket's own ring
(lib/util/xdpsock.c:1500-1548).

The sockets' batches lie one after the other: socket s owns flat records
base[s] .. base[s] + counts[s] - 1.  Packets are formed per socket; done[s] is
the index + 1 of the socket's last end-of-packet record, the records behind it
are its trailing incomplete packet and are processed by nothing.  Checked
against hand-written rows in test_socks_frags_abi.py; shared by the GPU tests."""
import numpy as np

from fragmodel import CONTD, frag_model
from sockmodel import bases, sock_model

PASS = 2
VERDICT_NONE = 0xff
PKT_NONE = 0xffffffff


def classify_model(counts, opts):
    """counts: records a socket; opts: u32 options in flat order.  Returns
    (done u32 [S], pkt_of u32 [n] with PKT_NONE, heads bool [n] -- the first
    records of the complete packets, in flat packet order --, (packets, records
    in them, trailing records))."""
    counts = np.asarray(counts, np.int64)
    opts = np.asarray(opts, np.uint32)
    base = bases(counts)
    n = int(base[-1])
    done = np.zeros(len(counts), np.uint32)
    pkt_of = np.full(n, PKT_NONE, np.uint32)
    heads = np.zeros(n, bool)
    packets = 0
    for s, c in enumerate(counts):
        b = int(base[s])
        p, h, (npk, dn, _) = frag_model(opts[b:b + int(c)])
        done[s] = dn
        pkt_of[b:b + dn] = p[:dn] + np.uint32(packets)
        heads[b:b + dn] = h[:dn]
        packets += npk
    recs = int(done.sum())
    return done, pkt_of, heads, (packets, recs, n - recs)


def live_mask(counts, done):
    """bool [n]: record i of socket s with i < done[s] (done None: all)."""
    counts = np.asarray(counts, np.int64)
    if done is None:
        return np.ones(int(counts.sum()), bool)
    local = np.arange(int(counts.sum())) - np.repeat(bases(counts)[:-1], counts)
    return local < np.repeat(np.asarray(done, np.int64), counts)


def spread(pkt_of, pv):
    """The verdict byte of every record from the packets' verdicts pv."""
    pv = np.asarray(pv, np.uint8)
    v = np.full(len(pkt_of), VERDICT_NONE, np.uint8)
    at = pkt_of != PKT_NONE
    v[at] = pv[pkt_of[at]]
    return v


def egress_model(counts, done, addr, lens, opts, v, has_tx=None, has_fill=None, shared=False):
    """sock_model over the live records: a TX record keeps XDP_PKT_CONTD in
    its options (the word behind len).  Returns (tx, fill, out) as sock_model,
    out[2s + 1] = done[s] - out[2s]."""
    counts = np.asarray(counts, np.int64)
    live = live_mask(counts, done)
    dn = counts if done is None else np.asarray(done, np.int64)
    word = np.asarray(lens).astype(np.uint64) | \
        ((np.asarray(opts).astype(np.uint64) & np.uint64(CONTD)) << np.uint64(32))
    return sock_model(dn, np.asarray(addr)[live], word[live], np.asarray(v)[live], has_tx, has_fill,
                      shared)


def swapped(counts, done, opts, v, has_tx=None):
    """bool [n]: the records XFG_EGRESS_SWAP_MACS touches -- live PASS records
    of a socket with a TX ring that start a packet."""
    counts = np.asarray(counts, np.int64)
    S = len(counts)
    has_tx = np.ones(S, bool) if has_tx is None else np.asarray(has_tx, bool)
    sock = np.repeat(np.arange(S), counts)
    first = np.zeros(len(sock), bool)
    first[bases(counts)[:-1][counts > 0]] = True
    eop = (np.asarray(opts, np.uint32) & CONTD) == 0
    head = first | np.concatenate([[False], eop[:-1]])[:len(sock)]
    return live_mask(counts, done) & (np.asarray(v) == PASS) & has_tx[sock] & head


def walk(counts, addr, lens, opts, pv, has_tx=None, has_fill=None, shared=False):
    """The same one record at a time: l2fwd() a socket.  pv: the verdict of
    every complete packet in flat packet order (its head record's).  Returns
    (done, pkt_of, verdicts, heads, (packets, records, trailing), tx, fill,
    out, swapped) as lists."""
    S = len(counts)
    n = int(sum(int(c) for c in counts))
    done, pkt_of, verd = [0] * S, [PKT_NONE] * n, [VERDICT_NONE] * n
    heads, swap = [False] * n, [False] * n
    tx, own, one = [[] for _ in range(S)], [[] for _ in range(S)], []
    out = [0] * (2 * S + 2)
    packets, i = 0, 0
    for s in range(S):
        frags = []                                 # the packet being collected: flat indices
        for j in range(int(counts[s])):
            frags.append(i)
            if not (int(opts[i]) & CONTD):         # IS_EOP_DESC: the packet is whole
                verdict = int(pv[packets])
                sent = verdict == PASS and (has_tx is None or bool(has_tx[s]))
                heads[frags[0]] = True
                swap[frags[0]] = sent
                for r in frags:
                    pkt_of[r], verd[r] = packets, verdict
                    if sent:
                        tx[s].append([int(addr[r]), int(lens[r]) | ((int(opts[r]) & CONTD) << 32)])
                        out[2 * s] += 1
                        out[2 * S] += 1
                    else:
                        out[2 * s + 1] += 1
                        out[2 * S + 1] += 1
                        if shared:
                            one.append(int(addr[r]) & (2**48 - 1))
                        elif has_fill is None or has_fill[s]:
                            own[s].append(int(addr[r]) & (2**48 - 1))
                packets += 1
                done[s] = j + 1
                frags = []
            i += 1
    recs = sum(done)
    return (done, pkt_of, verd, heads, (packets, recs, n - recs), tx, (one if shared else own), out,
            swap)

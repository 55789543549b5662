"""What xfg_socks_egress writes (include/xdpfilter_gpu.h), as a few lines of
numpy over the flat arrays, and the same as a plain walk over the records.

The sockets' batches lie one after the other: socket s owns flat records
base[s] .. base[s] + counts[s] - 1.  A record goes to its socket's TX ring if
its verdict is XDP_PASS and the socket has one (addr and len as received,
options 0); every other record hands its chunk address addr & (2^48 - 1) back,
to the shared fill ring in flat order or to its socket's own (none if the
socket has no fill ring).  Both return (tx, fill, out): tx[s] the [k, 2] u64 TX
records of socket s, fill the shared ring's addresses (shared) or the list of
every socket's, out the 2 * S + 2 counts."""
import numpy as np

PASS = 2
ADDR48 = np.uint64(2**48 - 1)


def bases(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def sock_model(counts, addr, lens, v, has_tx=None, has_fill=None, shared=False):
    counts = np.asarray(counts, np.int64)
    S = len(counts)
    has_tx = np.ones(S, bool) if has_tx is None else np.asarray(has_tx, bool)
    has_fill = np.ones(S, bool) if has_fill is None else np.asarray(has_fill, bool)
    sock = np.repeat(np.arange(S), counts)
    sent = (np.asarray(v) == PASS) & has_tx[sock]
    rec = np.stack([addr, lens.astype(np.uint64)], axis=1).astype(np.uint64).reshape(-1, 2)
    tx = [rec[sent & (sock == s)] for s in range(S)]
    back = addr & ADDR48
    if shared:
        fill = back[~sent]
    else:
        fill = [back[~sent & (sock == s)] if has_fill[s] else back[:0] for s in range(S)]
    nsent = np.bincount(sock[sent], minlength=S).astype(np.int64)
    out = np.empty(2 * S + 2, np.uint64)
    out[0:2 * S:2] = nsent
    out[1:2 * S:2] = counts - nsent
    out[2 * S] = nsent.sum()
    out[2 * S + 1] = counts.sum() - nsent.sum()
    return tx, fill, out


def walk(counts, addr, lens, v, has_tx=None, has_fill=None, shared=False):
    S = len(counts)
    tx = [[] for _ in range(S)]
    own = [[] for _ in range(S)]
    one = []
    out = [0] * (2 * S + 2)
    i = 0
    for s in range(S):
        for _ in range(int(counts[s])):
            if int(v[i]) == PASS and (has_tx is None or has_tx[s]):
                tx[s].append([int(addr[i]), int(lens[i])])
                out[2 * s] += 1
                out[2 * S] += 1
            else:
                out[2 * s + 1] += 1
                out[2 * S + 1] += 1
                if shared:
                    one.append(int(addr[i]) & (2**48 - 1))
                elif has_fill is None or has_fill[s]:
                    own[s].append(int(addr[i]) & (2**48 - 1))
            i += 1
    return tx, (one if shared else own), out

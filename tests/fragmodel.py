"""numpy model of multi-buffer RX batches (xfg_classify_descs_frags): which
records end a packet, each record's packet index, which records are heads, and
the three counts -- l2fwd()'s walk over a batch (lib/util/xdpsock.c:1500-1548:
nb_frags++ per record; at an end-of-packet record frags_done += nb_frags,
nb_frags = 0) stated over whole arrays.  Checked against hand-written rows in
test_frags_abi.py; shared by the GPU tests."""
import numpy as np

CONTD = 1      # XDP_PKT_CONTD, headers/linux/if_xdp.h:123


def frag_model(opts):
    """opts: u32 options of the batch's records in order.  Returns (pkt_of u32,
    heads bool, (packets, records in them, trailing records))."""
    opts = np.asarray(opts, np.uint32)
    n = len(opts)
    eop = (opts & CONTD) == 0
    inc = np.cumsum(eop, dtype=np.int64)
    pkt_of = (inc - eop).astype(np.uint32)                 # exclusive
    heads = np.concatenate([[True], eop[:-1]])[:n].astype(bool)
    at = np.flatnonzero(eop)
    done = int(at[-1]) + 1 if len(at) else 0
    return pkt_of, heads, (int(eop.sum()), done, n - done)


def walk(opts):
    """The same by l2fwd()'s loop, one record at a time."""
    pkt_of, heads, packets, nb_frags, frags_done, start = [], [], 0, 0, 0, True
    for o in opts:
        pkt_of.append(packets)
        heads.append(start)
        nb_frags += 1
        start = False
        if not (int(o) & CONTD):           # IS_EOP_DESC
            frags_done += nb_frags
            nb_frags = 0
            packets += 1
            start = True
    return pkt_of, heads, (packets, frags_done, len(opts) - frags_done)

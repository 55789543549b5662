"""Packet formation of xfg_capture_descs_frags (include/xdpfilter_gpu.h) from
the records' options and verdict bytes, stated once over whole arrays and once
as a record-at-a-time walk.  With n records:

    live[i] = v[i] != XFG_VERDICT_NONE
    eop[i]  = !(o[i] & XFG_XDP_PKT_CONTD)
    head[i] = live[i] and (i == 0 or not live[i-1] or eop[i-1])

The packet of head h is records h..e, e the smallest index >= h with eop[e];
it exists (is complete) only if every record h..e is live and e < n.  It is
selected by its head's verdict byte alone.  Checked against hand-written rows
in test_capture_frags_abi.py; shared by the GPU tests."""
import numpy as np

from capmodel import selected

CONTD = 1
VERDICT_NONE = 0xff
MASK_ALL = 0xffffffff


def form(opts, verdicts, mask=MASK_ALL):
    """Returns (heads, ends, complete, sel): the index of every head in order,
    its packet's last record (-1: the packet is not complete), and two bool
    arrays over the heads."""
    o = np.asarray(opts, np.uint32)
    v = np.asarray(verdicts, np.uint8)
    n = len(v)
    assert len(o) == n
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), np.zeros(0, bool), np.zeros(0, bool)
    live = v != VERDICT_NONE
    eop = (o & CONTD) == 0
    head = live.copy()
    head[1:] &= ~live[:-1] | eop[:-1]
    idx = np.arange(n, dtype=np.int64)
    # the first end-of-packet record, and the first record that is not live, at or after i
    nxt_eop = np.minimum.accumulate(np.where(eop, idx, n)[::-1])[::-1]
    nxt_dead = np.minimum.accumulate(np.where(live, n, idx)[::-1])[::-1]
    heads = np.flatnonzero(head).astype(np.int64)
    ends = nxt_eop[heads]
    complete = (ends < n) & (nxt_dead[heads] > ends)
    ends = np.where(complete, ends, -1)
    sel = complete & selected(v[heads], mask)
    return heads, ends, complete, sel


def walk(opts, verdicts, mask=MASK_ALL):
    """The same one record at a time, as lists."""
    heads, ends, complete, sel = [], [], [], []
    run = None                     # the head of the packet being collected
    for i in range(len(verdicts)):
        if int(verdicts[i]) == VERDICT_NONE:
            run = None             # (a run cut off here was recorded as not complete)
            continue
        if run is None:
            run = len(heads)
            heads.append(i)
            ends.append(-1)
            complete.append(False)
            sel.append(False)
        if not (int(opts[i]) & CONTD):
            vh = int(verdicts[heads[run]])
            ends[run], complete[run] = i, True
            sel[run] = vh < 32 and bool((mask >> vh) & 1)
            run = None
    return heads, ends, complete, sel

"""The model of a chained stage over a multi-buffer batch
(xfg_classify_descs_frags_chain; include/xdpfilter_gpu.h), stated once over
whole arrays on capfragmodel.form and once as a record-at-a-time walk in plain
Python.  Checked against each other and against hand-written rows in
test_frags_chain_abi.py; shared by the GPU tests.

Packets are formed as xfg_capture_descs_frags forms them (capfragmodel).  A
complete packet is selected by its head's verdict byte alone; the selected
packets' head records, in their order, are the plain descriptor array the
stage classifies, and every record of a selected packet gets its packet's new
verdict."""
import numpy as np

from capfragmodel import CONTD, VERDICT_NONE, form


def frags_chain_model(opts, verdicts, mask):
    """(idx, ends, counts): the selected packets' head record indices (u32,
    ascending), their end-of-packet records, and the call's three counts."""
    n = len(verdicts)
    heads, ends, _, sel = form(opts, verdicts, mask)
    idx, e = heads[sel].astype(np.uint32), ends[sel].astype(np.int64)
    recs = int((e - idx + 1).sum())
    return idx, e, (len(idx), recs, n - recs)


def heads_of_records(records, idx):
    """The selected packets' head records (batch order: the ring unrolled)."""
    return np.asarray(records, np.uint64).reshape(-1, 2)[idx]


def merge(old, idx, ends, new):
    """The verdict bytes after the stage: new[k] on records idx[k]..ends[k],
    the rest as before."""
    out = np.array(old, np.uint8, copy=True)
    if len(idx):
        reps = np.asarray(ends, np.int64) - np.asarray(idx, np.int64) + 1
        starts = np.repeat(np.asarray(idx, np.int64), reps)
        within = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
        out[starts + within] = np.repeat(np.asarray(new, np.uint8), reps)
    return out


def walk(opts, verdicts, mask, new=None):
    """The same one record at a time: (idx, ends, counts, merged verdicts or
    None), as lists."""
    n = len(verdicts)
    idx, ends, out = [], [], [int(v) for v in verdicts]
    head = None                      # the head of the live run being collected
    recs = 0
    for i in range(n):
        if int(verdicts[i]) == VERDICT_NONE:
            head = None              # a run cut off here was no packet
            continue
        if head is None:
            head = i
        if int(opts[i]) & CONTD:
            continue
        vh = int(verdicts[head])
        if vh < 32 and (int(mask) >> vh) & 1:
            if new is not None:
                for r in range(head, i + 1):
                    out[r] = int(new[len(idx)])
            idx.append(head)
            ends.append(i)
            recs += i - head + 1
        head = None                  # the next live record starts a packet
    return idx, ends, (len(idx), recs, n - recs), out if new is not None else None

"""The numpy model of a chained stage (xfg_classify_chain,
xfg_classify_descs_chain; include/xdpfilter_gpu.h), shared by the CPU test
that checks it against a per-frame loop and by the GPU tests.

Frame i is selected if its verdict byte v is below 32 and bit v of the chain
mask is set.  The selected frames, in their order, are a plain array of
struct xdp_desc records {u64 addr; u32 len; u32 options}, here rows of two
u64 (addr, len | options << 32): a descriptor batch's records as received, a
batch's frames as {byte offset, length (bounded by the slot for a fixed
stride), options 0}."""
import numpy as np


def selected(verdicts, mask):
    """The selected frames' indices, ascending (u32)."""
    v = np.asarray(verdicts, np.uint8).astype(np.uint32)
    bit = (np.uint32(mask) >> np.minimum(v, 31)) & 1
    return np.flatnonzero((v < 32) & (bit == 1)).astype(np.uint32)


def descs_of_records(records, idx):
    """A descriptor batch's selected records (batch order: the ring unrolled)."""
    return np.asarray(records, np.uint64).reshape(-1, 2)[idx]


def descs_of_batch(lens, idx, stride=0, offsets=None):
    """A struct xfg_batch's selected frames as plain descriptors."""
    lens = np.asarray(lens).astype(np.uint64)
    idx = np.asarray(idx, np.uint32)
    d = np.zeros((len(idx), 2), np.uint64)
    if offsets is None:
        d[:, 0] = idx.astype(np.uint64) * np.uint64(stride)
        d[:, 1] = np.minimum(lens[idx], np.uint64(stride))
    else:
        d[:, 0] = np.asarray(offsets, np.uint64)[idx]
        d[:, 1] = lens[idx]
    return d


def merge(old, idx, new):
    """The verdict bytes after the stage: new[k] at idx[k], the rest as before."""
    out = np.array(old, np.uint8, copy=True)
    out[idx] = new
    return out


def chain_model(verdicts, mask):
    """(idx, counts) of a stage over these verdict bytes."""
    idx = selected(verdicts, mask)
    return idx, (len(idx), len(verdicts) - len(idx))


def walk(verdicts, mask, lens, stride=0, offsets=None, new=None):
    """The same, frame by frame in plain Python: (idx, descriptors as (addr,
    len, options) tuples, merged verdicts or None)."""
    idx, descs, out, k = [], [], [int(v) for v in verdicts], 0
    for i, v in enumerate(verdicts):
        v = int(v)
        if v >= 32 or not (int(mask) >> v) & 1:
            continue
        idx.append(i)
        if offsets is None:
            descs.append((i * stride, min(int(lens[i]), stride), 0))
        else:
            descs.append((int(offsets[i]), int(lens[i]), 0))
        if new is not None:
            out[i] = int(new[k])
        k += 1
    return idx, descs, out if new is not None else None

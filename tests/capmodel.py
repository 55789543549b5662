"""A struct-packing model of the capture format (include/xdpfilter_io.h,
xfg_pcapng_write_captured): the section and interface blocks and the Enhanced
Packet Block with the epb_verdict option, little endian.  Shared by the CPU
tests, which pin the library's writer to it, and the GPU tests, which compare
the device's blocks with that writer's."""
import struct

import numpy as np

APPL = b"xdp-filter (MI355X classifier)"
MASK_ALL = 0xffffffff


def _opt(code, payload):
    return struct.pack("<HH", code, len(payload)) + payload + bytes(-len(payload) % 4)


def _block(btype, body):
    total = 12 + len(body)
    return struct.pack("<II", btype, total) + body + struct.pack("<I", total)


def preamble(ifname="xdp", snaplen=0):
    shb = _block(0x0A0D0D0A, struct.pack("<IHHq", 0x1A2B3C4D, 1, 0, -1) + _opt(4, APPL) +
                 struct.pack("<I", 0))
    idb = _block(1, struct.pack("<HHI", 1, 0, snaplen) + _opt(2, ifname.encode()) +
                 _opt(9, b"\x09") + struct.pack("<I", 0))
    return shb + idb


def epb(frame, verdict, snaplen=0, orig_len=None, ts=0):
    """The block of one frame: {6, L, 0, ts >> 32, (u32)ts, cap, len}, cap
    bytes padded to 4, option {7, 9, 2, u64 verdict, 3 zero bytes}, {0}, L."""
    frame = bytes(frame)
    cap = min(len(frame), snaplen) if snaplen else len(frame)
    cap4 = (cap + 3) & ~3
    L = 52 + cap4
    out = (struct.pack("<7I", 6, L, 0, ts >> 32, ts & 0xffffffff, cap,
                       len(frame) if orig_len is None else orig_len) +
           frame[:cap] + bytes(cap4 - cap) + struct.pack("<HHBQ3x", 7, 9, 2, verdict) +
           struct.pack("<II", 0, L))
    assert len(out) == L
    return out


def selected(verdicts, mask):
    v = np.asarray(verdicts).astype(np.int64)
    return (v < 32) & (((mask >> np.minimum(v, 31)) & 1) == 1)


def blocks(frames, verdicts, mask, snaplen=0, orig_lens=None, ts_ns=None):
    """The blocks, one bytes object each, of the selected frames in packet order."""
    sel = selected(verdicts, mask)
    return [epb(f, int(verdicts[i]), snaplen, None if orig_lens is None else int(orig_lens[i]),
                0 if ts_ns is None else int(ts_ns[i]))
            for i, f in enumerate(frames) if sel[i]]

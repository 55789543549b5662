"""Capture by verdict on the device (xfg_capture, xfg_capture_descs,
xfg_capture.hip): the selected frames of a device batch as pcapng blocks.

Every comparison is exact.  The expected bytes are the EPBs that
xfg_pcapng_write_captured() writes for the same frames, verdicts, mask and
snap length (test_capture_io.py pins that writer to the struct-packing model);
the lengths of the blocks, for the overflow cases, are worked out again here
in numpy.  The output buffer is compared whole -- 0xA5 bytes with the expected
prefix written in, and a guard past out_bytes -- so nothing at or past
counts[1] may change.
"""
import functools
import os
import re
import tempfile

import numpy as np
import pytest

import capmodel as M
import xftools as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABORTED, DROP, PASS = 0, 1, 2
MASK_DROP, MASK_AD = 1 << DROP, 1 << DROP | 1 << ABORTED
BYTES = np.array([0, 1, 2, 3, 4, 31, 32, 255], np.uint8)   # verdict bytes the batches carry
SNAPS = [0, 1, 60, 64, 65, 96, 1514]
PATTERNS = ["random", "all", "none", "alternating", "tile_last", "first", "last"]
EDGE_LENS = np.array([0, 1, 2, 3, 4, 13, 14, 59, 60, 61, 63, 64, 65, 66, 95, 96, 97, 1513, 1514],
                     np.uint32)
CHUNK, NCHUNKS = 2048, 4096
GUARD = 256
A5 = 0xA5


def tile():
    src = open(os.path.join(ROOT, "xdp-tools_amd", "csrc", "xfg_layout.h")).read()
    return int(re.search(r"#define\s+XFG_CAPTURE_TILE\s+(\d+)u", src).group(1))


T = tile()
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7, 2**20 + 13]
BIG = 2**22 + 13     # more tiles than workgroups on any device: every workgroup loops


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def umem():
    u = np.random.default_rng(11).integers(0, 256, NCHUNKS * CHUNK, dtype=np.uint8)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=4)
def frames_of(n):
    """n frames in the UMEM (read only): chunk, headroom 0 / 16 / 256 and a
    length 0..1514, half of them from the edge lengths.  Frames alias (n may
    be far above the chunk count): nothing writes the UMEM."""
    rng = np.random.default_rng(3000 + n)
    chunk = rng.integers(0, NCHUNKS, n).astype(np.uint64)
    head = np.choose(np.arange(n) % 3, [0, 256, 16]).astype(np.uint64)
    lens = rng.integers(0, 1515, n).astype(np.uint32)
    edge = rng.random(n) < 0.5
    lens[edge] = EDGE_LENS[rng.integers(0, len(EDGE_LENS), int(edge.sum()))]
    ts = np.uint64(1_700_000_000_000_000_000) + rng.integers(0, 2**40, n).astype(np.uint64)
    for a in (chunk, head, lens, ts):
        a.setflags(write=False)
    return chunk, head, lens, ts


@functools.lru_cache(maxsize=None)
def verdicts_of(n, pattern, sel=DROP, frac=0.5):
    """Verdict bytes of every kind; @sel where the pattern selects."""
    rng = np.random.default_rng(16 * n + PATTERNS.index(pattern))
    others = BYTES[BYTES != sel]
    v = others[rng.integers(0, len(others), n)]
    if pattern == "random":
        v[rng.random(n) < frac] = sel
    elif pattern == "all":
        v[:] = sel
    elif pattern == "alternating":
        v[0::2] = sel
    elif pattern == "tile_last":
        v[T - 1::T] = sel
    elif pattern == "first":
        v[:1] = sel
    elif pattern == "last":
        v[n - 1:] = sel
    v.setflags(write=False)
    return v


def reference(data, offs, lens, v, mask, snaplen, ts):
    """The EPB bytes of xfg_pcapng_write_captured for a host batch."""
    import xfgpu as G
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ref.pcapng")
        G.pcapng_write_captured(path, None, data, offs, lens, v, mask, snaplen, ts_ns=ts)
        blob = np.fromfile(path, np.uint8)
    pre = len(M.preamble("xdp", snaplen))
    assert blob[:pre].tobytes() == M.preamble("xdp", snaplen)
    return blob[pre:]


def block_lens(lens, v, mask, snaplen):
    cap = np.minimum(lens, snaplen) if snaplen else lens
    return (52 + ((cap.astype(np.int64) + 3) & ~3))[M.selected(v, mask)]


class Source:
    """One batch on the device in a given form, and the host batch the
    reference writer reads (data, offsets, lens)."""

    def __init__(self, G, f, n, form):
        self.f, self.n, self.bufs = f, n, []
        chunk, head, lens, self.ts = frames_of(n)
        if form in ("stride64", "stride2048"):
            stride = 64 if form == "stride64" else CHUNK
            rng = np.random.default_rng(77 + n)
            self.data = rng.integers(0, 256, max(n, 1) * stride, dtype=np.uint8)
            self.offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
            self.lens = np.minimum(lens, 64) if stride == 64 else lens.copy()
            d_lens = self.lens.astype(np.uint16) if form == "stride2048" else self.lens
            self.batch = G.Batch(self.up(self.data, 64), None, self.up(d_lens), n, stride,
                                 int(d_lens.dtype == np.uint16))
        elif form in ("offsets_u32", "offsets_u16"):
            self.data, self.offs, self.lens = umem(), chunk * np.uint64(CHUNK) + head, lens.copy()
            d_lens = self.lens.astype(np.uint16) if form == "offsets_u16" else self.lens
            self.batch = G.Batch(self.up(self.data, 64), self.up(self.offs), self.up(d_lens), n, 0,
                                 int(d_lens.dtype == np.uint16))
        else:
            # descriptors: every third address in the unaligned-chunk form; a
            # plain array, or a ring whose first wraps it (and, from 64
            # packets on, the u32 index itself)
            self.data, self.offs, self.lens = umem(), chunk * np.uint64(CHUNK) + head, lens.copy()
            base = chunk * np.uint64(CHUNK)
            addr = np.where(np.arange(n) % 3 == 2, base | (head << np.uint64(48)), base + head)
            if form == "descs_array":
                entries, first, mask = n + 3, 0, 0xffffffff
            else:
                entries = 16
                while entries < n:
                    entries *= 2
                first, mask = (0xfffffff0 if n >= 64 else entries - n // 2 - 1), entries - 1
            rec = np.full((entries, 2), 0xA5A5A5A5A5A5A5A5, np.uint64)
            slot = ((first + np.arange(n, dtype=np.uint64)) & np.uint64(0xffffffff)
                    & np.uint64(mask)).astype(np.int64)
            rec[slot, 0] = addr
            rec[slot, 1] = self.lens.astype(np.uint64) | np.uint64(0x10000 << 32)   # option bits
            self.batch = G.DescBatch(self.up(self.data, 64), self.up(rec), first, mask, n)

    def up(self, arr, slack=0):
        b = self.f.alloc(max(arr.nbytes, 16) + slack)
        b.upload(arr)
        self.bufs.append(b)
        return b.ptr

    def free(self):
        for b in self.bufs:
            b.free()


def run_capture(G, f, src, v, mask, snaplen, with_ts, out_bytes=None, ts0=0, stream=None):
    """One call; checks the three counts and the whole output buffer.
    out_bytes: a number, or a function of the total (None: the total)."""
    n = src.n
    ts = src.ts if with_ts else None
    want = reference(src.data, src.offs, src.lens, v, mask, snaplen,
                     ts if with_ts else np.full(n, ts0, np.uint64))
    L = block_lens(src.lens, v, mask, snaplen)
    ends = np.cumsum(L)
    total = int(ends[-1]) if len(L) else 0
    assert total == len(want)
    room = total if out_bytes is None else out_bytes(total) if callable(out_bytes) else out_bytes
    written = int(np.searchsorted(ends, room, side="right"))
    nbytes = int(ends[written - 1]) if written else 0
    size = (room + 15) // 16 * 16 + GUARD
    d_out, d_c, d_v = f.alloc(size), f.alloc(32), f.alloc(max(n, 16))
    d_ts = f.alloc(max(8 * n, 16)) if with_ts else None
    try:
        d_out.upload(np.full(size, A5, np.uint8))
        d_c.upload(np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64))
        if n:
            d_v.upload(v)
        if with_ts and n:
            d_ts.upload(ts)
        f.sync()
        f.capture_into(src.batch, d_v.ptr, mask, d_out.ptr, room, d_c.ptr, snaplen=snaplen,
                       ts_ns_ptr=d_ts.ptr if with_ts else None, ts0=ts0, stream=stream)
        f.sync()
        counts = d_c.download(np.zeros(3, np.uint64)).tolist()
        got = d_out.download(np.zeros(size, np.uint8))
    finally:
        for b in (d_out, d_c, d_v, d_ts):
            if b:
                b.free()
    print(f"n {n} selected {len(L)} total {total} room {room} counts {counts}")
    assert counts == [written, nbytes, len(L) - written]
    expect = np.full(size, A5, np.uint8)
    expect[:nbytes] = want[:nbytes]
    assert np.array_equal(got, expect), first_difference(got, expect)
    return got[:nbytes]


def first_difference(got, expect):
    at = np.flatnonzero(got != expect)
    return f"{len(at)} bytes differ, the first at {at[0]}: {got[at[0]]:#x} for {expect[at[0]]:#x}"


# ---- 1: sizes x selection patterns (descriptor rings that wrap)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_patterns(G, filt, n, pattern):
    k = PATTERNS.index(pattern)
    # (1514 bytes of 2^20 frames would be gigabytes: the largest n takes the short snaps)
    snaplen = [96, 1, 60, 64, 65, 96, 60][k] if n > 2**16 else SNAPS[(k + SIZES.index(n)) % 7]
    src = Source(G, filt, n, "descs_ring")
    try:
        run_capture(G, filt, src, verdicts_of(n, pattern), MASK_DROP, snaplen, with_ts=k % 2 == 0,
                    ts0=0x1122334455667788)
    finally:
        src.free()


def test_every_workgroup_loops(G, filt):
    """More tiles than resident workgroups: each takes several, and the
    look-back runs across all of them (one frame in ten, one payload byte)."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert (BIG + T - 1) // T > 4 * ncu
    src = Source(G, filt, BIG, "descs_array")
    try:
        run_capture(G, filt, src, verdicts_of(BIG, "random", DROP, 0.1), MASK_DROP, 1, with_ts=True)
    finally:
        src.free()


# ---- 2: source forms x snap lengths
@pytest.mark.parametrize("snaplen", SNAPS)
@pytest.mark.parametrize("form", ["stride64", "stride2048", "offsets_u32", "offsets_u16",
                                  "descs_array", "descs_ring"])
def test_forms_and_snaplens(G, filt, form, snaplen):
    for n in (T + 1, 3 * T + 7):
        src = Source(G, filt, n, form)
        try:
            run_capture(G, filt, src, verdicts_of(n, "random"), MASK_DROP, snaplen,
                        with_ts=SNAPS.index(snaplen) % 2 == 1, ts0=5)
        finally:
            src.free()


def test_stride64_large(G, filt):
    """C3's layout at the largest size, whole frames."""
    n = SIZES[-1]
    src = Source(G, filt, n, "stride64")
    try:
        run_capture(G, filt, src, verdicts_of(n, "random"), MASK_DROP, 0, with_ts=False, ts0=1 << 40)
    finally:
        src.free()


# ---- 3: the mask
@pytest.mark.parametrize("mask", [MASK_AD, 1 << PASS, 1 << 4 | 1 << 31, M.MASK_ALL])
def test_masks(G, filt, mask):
    """Bit a selects verdict byte a; bytes 32 and 255 are never selected."""
    n = 3 * T + 7
    v = BYTES[np.random.default_rng(5).integers(0, len(BYTES), n)]
    assert set(np.unique(v[M.selected(v, M.MASK_ALL)])) == {0, 1, 2, 3, 4, 31}
    src = Source(G, filt, n, "offsets_u32")
    try:
        run_capture(G, filt, src, v, mask, 96, with_ts=True)
    finally:
        src.free()


@pytest.mark.parametrize("form", ["stride64", "descs_ring"])
def test_empty_results(G, filt, form):
    """action_mask == 0, or count == 0: three zero counts and nothing else
    (the verdicts may then be absent)."""
    for n, mask in ((3 * T + 7, 0), (0, MASK_DROP), (0, 0)):
        src = Source(G, filt, n, form)
        try:
            run_capture(G, filt, src, verdicts_of(n, "all"), mask, 0, with_ts=False)
        finally:
            src.free()
    d_c = filt.alloc(32)
    d_c.upload(np.full(3, 7, np.uint64))
    b = G.DescBatch(None, None, 0, 0xffffffff, 0)
    filt.capture_into(b, None, MASK_DROP, None, 0, d_c.ptr)
    filt.sync()
    assert d_c.download(np.zeros(3, np.uint64)).tolist() == [0, 0, 0]
    d_c.free()


# ---- 4: overflow
ROOMS = {"0": 0, "51": 51, "total-1": lambda t: t - 1, "total": lambda t: t,
         "total+16": lambda t: t + 16, "half": lambda t: t // 2 + 3}


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("n", [65, 3 * T + 7])
@pytest.mark.parametrize("form,snaplen", [("descs_ring", 0), ("offsets_u16", 65)])
def test_overflow_writes_a_prefix(G, filt, form, snaplen, n, room):
    """A block is written only if it ends at or before out_bytes; a later,
    smaller frame is not slipped in; bytes from counts[1] on are untouched."""
    src = Source(G, filt, n, form)
    try:
        run_capture(G, filt, src, verdicts_of(n, "random"), MASK_AD, snaplen, with_ts=True,
                    out_bytes=ROOMS[room])
    finally:
        src.free()


def test_overflow_does_not_slip_a_smaller_frame_in(G, filt):
    """Room for the first block and 60 bytes: the second block (1514 bytes)
    does not fit, the third (56 bytes) would."""
    n = 3
    lens = np.array([64, 1514, 1], np.uint32)
    src = Source(G, filt, n, "offsets_u32")
    src.lens = lens
    src.batch.lens = src.up(lens)
    try:
        got = run_capture(G, filt, src, np.full(n, DROP, np.uint8), MASK_DROP, 0, with_ts=False,
                          out_bytes=116 + 60)
        assert len(got) == 116
    finally:
        src.free()


# ---- 5: stream order after classify_descs; the call is inert
STRIDE = 160


@pytest.fixture(scope="module")
def classified(G):
    """A small mixed rule set, 4,097 fuzz frames in a UMEM, the oracle's
    verdicts, and a context with the rules loaded."""
    from test_gpu_descs import ring_of, umem_of
    rules, pool = X.random_rules(77, n4=200, n6=80, ne=24, nports=40)
    data, lens = X.gen_fuzz(31, 4097, STRIDE, rules, pool)
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    ov, _, _ = X.run_oracle(feats, data, lens, rules, stride=STRIDE)
    assert 0 < np.count_nonzero(ov == DROP) < len(ov)
    um, addr = umem_of(data, lens, STRIDE, seed=5)
    descs, first, mask = ring_of(addr, lens, 8192, 8192 - 777, fill=0xFF)
    f = G.Filter(feats, ndev=1, descs_min_packets=1)
    f.load_rules(rules)
    yield f, rules, data, um, lens, descs, first, mask, ov
    f.close()


def state_of(G, f, rules):
    r = rules.prepared()
    return [f.stats().copy(), f.values_of(G.MAP_IPV4, r.v4_keys), f.values_of(G.MAP_IPV6, r.v6_keys),
            f.values_of(G.MAP_ETHERNET, r.eth_keys),
            f.values_of(G.MAP_PORTS, np.arange(65536, dtype=np.uint32))]


@pytest.mark.parametrize("where", ["library_stream", "caller_stream"])
def test_classify_then_capture_without_sync(G, classified, where):
    import torch
    f, rules, data, um, lens, descs, first, mask, ov = classified
    n = len(lens)
    stream = torch.cuda.Stream() if where == "caller_stream" else None
    sp = stream.cuda_stream if stream else None
    offs = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    room = 1 << 23
    d_u, d_rx, d_v = f.alloc(um.nbytes + 64), f.alloc(descs.nbytes), f.alloc(n)
    d_out, d_c = f.alloc(room), f.alloc(32)
    d_u.upload(um)
    d_rx.upload(descs)
    d_v.upload(np.full(n, 255, np.uint8))
    d_out.upload(np.full(room, A5, np.uint8))
    f.sync()
    b = G.DescBatch(d_u.ptr, d_rx.ptr, first, mask, n)
    f.classify_descs(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask, stream=sp)
    f.capture_into(b, d_v.ptr, MASK_AD, d_out.ptr, room, d_c.ptr, snaplen=96, ts0=42, stream=sp)
    if stream:
        stream.synchronize()
    f.sync()
    v = d_v.download(np.zeros(n, np.uint8))
    np.testing.assert_array_equal(v, ov)
    # the blob built from the verdicts read back
    want = reference(data, offs, lens, v, MASK_AD, 96, np.full(n, 42, np.uint64))
    counts = d_c.download(np.zeros(3, np.uint64)).tolist()
    assert counts == [int(np.count_nonzero(M.selected(v, MASK_AD))), len(want), 0]
    expect = np.full(room, A5, np.uint8)
    expect[:len(want)] = want
    assert np.array_equal(d_out.download(np.zeros(room, np.uint8)), expect)
    for buf in (d_u, d_rx, d_v, d_out, d_c):
        buf.free()


def test_capture_is_inert(G, classified):
    """Map values and statistics before and after a capture are equal."""
    f, rules, data, um, lens, descs, first, mask, ov = classified
    n = len(lens)
    d_u, d_rx, d_v = f.alloc(um.nbytes + 64), f.alloc(descs.nbytes), f.alloc(n)
    d_u.upload(um)
    d_rx.upload(descs)
    d_v.upload(ov)
    before = state_of(G, f, rules)
    b = G.DescBatch(d_u.ptr, d_rx.ptr, first, mask, n)
    blocks, written, lost = f.capture_descs(b, d_v.ptr, M.MASK_ALL, snaplen=0, out_bytes=1 << 22)
    assert (written, lost) == (n, 0)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE)
    assert np.array_equal(blocks, reference(data, offs, lens, ov, M.MASK_ALL, 0, np.zeros(n, np.uint64)))
    for x, y in zip(before, state_of(G, f, rules)):
        np.testing.assert_array_equal(x, y)
    for buf in (d_u, d_rx, d_v):
        buf.free()


# ---- 6: the binding's convenience calls, and a file built from them
def test_capture_returns_blocks_written_lost(G, filt, tmp_path):
    n = 3 * T + 7
    v = verdicts_of(n, "random")
    src = Source(G, filt, n, "offsets_u32")
    d_v, d_ts = filt.alloc(n), filt.alloc(8 * n)
    d_v.upload(v)
    d_ts.upload(src.ts)
    try:
        want = reference(src.data, src.offs, src.lens, v, MASK_DROP, 60, src.ts)
        blocks, written, lost = filt.capture(src.batch, d_v.ptr, MASK_DROP, snaplen=60,
                                             out_bytes=1 << 20, ts_ns=d_ts.ptr)
        nsel = int(np.count_nonzero(v == DROP))
        assert (written, lost) == (nsel, 0) and blocks.dtype == np.uint8
        assert np.array_equal(blocks, want)
        # too little room: a prefix, and the rest counted
        few, written, lost = filt.capture(src.batch, d_v.ptr, MASK_DROP, snaplen=60,
                                          out_bytes=112 * 10 + 50, ts_ns=d_ts.ptr)
        ends = np.cumsum(block_lens(src.lens, v, MASK_DROP, 60))
        fit = int(np.searchsorted(ends, 112 * 10 + 50, side="right"))
        assert (written, lost) == (fit, nsel - fit) and 0 < fit < nsel
        assert np.array_equal(few, want[:int(ends[fit - 1])])
        # begin + append of the device's blocks is the file of the CPU writer
        path, ref = tmp_path / "dev.pcapng", tmp_path / "cpu.pcapng"
        G.pcapng_begin(path, "veth0", 60)
        G.pcapng_append(path, blocks)
        G.pcapng_write_captured(ref, "veth0", src.data, src.offs, src.lens, v, MASK_DROP, 60,
                                ts_ns=src.ts)
        assert path.read_bytes() == ref.read_bytes()
        rdata, roffs, rlens, rorig, rts = G.read_pcap(path)
        sel = v == DROP
        assert rlens.tolist() == np.minimum(src.lens[sel], 60).tolist()
        assert rorig.tolist() == src.lens[sel].tolist() and rts.tolist() == src.ts[sel].tolist()
    finally:
        src.free()
        d_v.free()
        d_ts.free()


# ---- 7: the status words shared with xfg_compact
def test_scratch_shared_with_compact(G, filt):
    """compact, capture, compact, capture back to back without a sync, of
    sizes whose tile counts differ both ways."""
    f = filt
    sizes = [3 * 65536 + 7, 100003, 50001, 2**18 + 1]
    held, jobs = [], []
    for k, n in enumerate(sizes):
        v = verdicts_of(n, "random", DROP, 0.1)
        d_v, d_c = f.alloc(n), f.alloc(32)
        d_v.upload(v)
        held += [d_v, d_c]
        if k % 2 == 0:
            d_i = f.alloc(4 * n)
            held.append(d_i)
            jobs.append(("compact", n, v, d_v, d_c, d_i))
        else:
            src = Source(G, f, n, "descs_array")
            d_o = f.alloc(1 << 22)
            held.append(d_o)
            jobs.append(("capture", n, v, d_v, d_c, src, d_o))
    f.sync()
    for job in jobs:
        if job[0] == "compact":
            _, n, v, d_v, d_c, d_i = job
            f.compact(d_v.ptr, n, DROP, d_i.ptr, d_c.ptr)
        else:
            _, n, v, d_v, d_c, src, d_o = job
            f.capture_into(src.batch, d_v.ptr, MASK_DROP, d_o.ptr, 1 << 22, d_c.ptr, snaplen=64)
    f.sync()
    for job in jobs:
        if job[0] == "compact":
            _, n, v, d_v, d_c, d_i = job
            want = np.flatnonzero(v == DROP).astype(np.uint32)
            assert int(d_c.download(np.zeros(1, np.uint64))[0]) == len(want)
            np.testing.assert_array_equal(d_i.download(np.zeros(len(want), np.uint32)), want)
        else:
            _, n, v, d_v, d_c, src, d_o = job
            want = reference(src.data, src.offs, src.lens, v, MASK_DROP, 64,
                             np.zeros(n, np.uint64))
            assert d_c.download(np.zeros(3, np.uint64)).tolist() == [int((v == DROP).sum()),
                                                                      len(want), 0]
            assert np.array_equal(d_o.download(np.zeros(len(want), np.uint8)), want)
            src.free()
    for b in held:
        b.free()

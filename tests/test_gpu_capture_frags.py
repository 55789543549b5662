"""Capture by verdict of multi-buffer AF_XDP packets on the device
(xfg_capture_descs_frags, xfg_capture_frags.hip): one pcapng block a packet.

Every comparison is exact.  The expected bytes are the EPBs that
xfg_pcapng_write_captured() writes (test_capture_io.py pins that writer to the
struct-packing model) for a host batch whose frames are the packets'
concatenated bytes -- or their head records' with XFG_CAPTURE_HEAD_ONLY --,
whose verdicts are the heads' verdict bytes and whose timestamps the heads';
the packets are those of capfragmodel.form (test_capture_frags_abi.py checks
it).  The host batch is gathered from the UMEM in numpy, no loop over packets.
The output buffer is compared whole -- 0xA5 bytes with the expected prefix
written in, and a guard past out_bytes -- so nothing at or past counts[1] may
change.
"""
import functools
import os
import tempfile

import numpy as np
import pytest

import capfragmodel as CM
import capmodel as M
import xftools as X
from test_gpu_capture import A5, CHUNK, GUARD, NCHUNKS, T, first_difference, state_of, umem

pytestmark = pytest.mark.gpu

ABORTED, DROP, PASS = 0, 1, 2
MASK_DROP, MASK_AD = 1 << DROP, 1 << DROP | 1 << ABORTED
NONE = CM.VERDICT_NONE
CONTD = CM.CONTD
BYTES = np.array([0, 1, 2, 3, 4, 31, 32, 254], np.uint8)   # verdict bytes of live records
LENSET = np.array([0, 1, 2, 3, 4, 5, 7, 13, 60, 63, 64, 65, 1513, 1514, 2048], np.int64)
SNAPS = [0, 1, 60, 64, 65, 96, 1514, 4000]
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]
BIG = 2**22 + 13     # more tiles than workgroups on any device: every workgroup loops
HEAD_ONLY = 1


@pytest.fixture(scope="module")
def G():
    import xfgpu
    assert xfgpu.CAPTURE_HEAD_ONLY == HEAD_ONLY
    return xfgpu


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


@pytest.fixture(scope="module")
def d_um(filt):
    """The UMEM of test_gpu_capture.py (4096 chunks of 2048 bytes, read only) on the device."""
    b = filt.alloc(NCHUNKS * CHUNK + 64)
    b.upload(umem())
    filt.sync()
    yield b
    b.free()


# ---- batches
def shapes(rng, n, single=0.25):
    """XDP_PKT_CONTD of n records in packets of 1-5 records, one in four a
    single; the last packet is cut off where the batch ends."""
    k = np.where(rng.random(n + 1) < single, 1, rng.integers(2, 6, n + 1))
    ends = np.cumsum(k) - 1
    c = np.ones(n, np.uint32)
    c[ends[ends < n]] = 0
    return c


def with_bits(cont):
    """Option words: CONTD and, on some records, bits that mean nothing."""
    n = len(cont)
    return (cont | np.where(np.arange(n) % 5 == 4, 0x10000, 0) |
            np.where(np.arange(n) % 7 == 3, 0xfffe0000, 0)).astype(np.uint32)


def places(rng, n, lens=None):
    """n records in the UMEM: chunk, headroom 0 / 256 / 16, a length of the
    set (2048 stands for what the headroom leaves), a timestamp."""
    chunk = rng.integers(0, NCHUNKS, n).astype(np.int64)
    head = np.choose(np.arange(n) % 3, [0, 256, 16]).astype(np.int64)
    if lens is None:
        lens = LENSET[rng.integers(0, len(LENSET), n)]
    lens = np.minimum(np.asarray(lens, np.int64), CHUNK - head)
    ts = np.uint64(1_700_000_000_000_000_000) + rng.integers(0, 2**40, n).astype(np.uint64)
    return chunk, head, lens, ts


def verdict_bytes(rng, cont, sel=DROP, frac=0.5):
    """A byte of BYTES a record; a head's is @sel with probability frac, and a
    record that is no head carries a byte that differs from its head's."""
    n = len(cont)
    v = BYTES[rng.integers(0, len(BYTES), n)]
    head = np.ones(n, bool)
    head[1:] = cont[:-1] == 0
    v[head & (rng.random(n) < frac)] = sel
    hv = v[np.maximum.accumulate(np.where(head, np.arange(n), 0))] if n else v
    same = ~head & (v == hv)
    v[same] = np.where(hv[same] == PASS, 3, PASS)
    return v


class Recs:
    """n records on the device as a plain array or a ring whose first wraps it
    (and, from 64 records on, the u32 index itself); every third address in
    the unaligned-chunk form."""

    def __init__(self, G, f, d_um, chunk, head, lens, opts, ts, ring=False):
        n = len(lens)
        self.f, self.n, self.bufs = f, n, []
        self.off = chunk * CHUNK + head
        self.lens, self.opts, self.ts = np.asarray(lens, np.int64), np.asarray(opts, np.uint32), ts
        base = (chunk * CHUNK).astype(np.uint64)
        addr = np.where(np.arange(n) % 3 == 2, base | (head.astype(np.uint64) << np.uint64(48)),
                        base + head.astype(np.uint64))
        if not ring:
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
        rec[slot, 1] = self.lens.astype(np.uint64) | (self.opts.astype(np.uint64) << np.uint64(32))
        self.d_rec = self.up(rec)
        self.batch = G.DescBatch(d_um.ptr, self.d_rec, first, mask, n)

    def up(self, arr):
        b = self.f.alloc(max(arr.nbytes, 16))
        b.upload(arr)
        self.bufs.append(b)
        return b.ptr

    def free(self):
        for b in self.bufs:
            b.free()


def make(G, f, d_um, n, seed, ring=False, lens=None, cont=None):
    rng = np.random.default_rng(seed)
    cont = shapes(rng, n) if cont is None else np.asarray(cont, np.uint32)
    chunk, head, lens, ts = places(rng, n, lens)
    return Recs(G, f, d_um, chunk, head, lens, with_bits(cont), ts, ring), rng


# ---- the reference
def gather(um, off, lens, h, e, limit=None):
    """The frames of packets h[k]..e[k]: their records' bytes in order, at
    most @limit of each.  Returns (data, frame lengths)."""
    if not len(h):
        return np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    nrec = e - h + 1
    first = np.cumsum(nrec) - nrec
    rec = np.repeat(h - first, nrec) + np.arange(int(nrec.sum()))
    rl = lens[rec]
    cs = np.cumsum(rl) - rl
    before = cs - np.repeat(cs[first], nrec)       # the packet's bytes before the record
    take = rl if limit is None else np.clip(limit - before, 0, rl)
    start = np.cumsum(take) - take
    src = np.repeat(off[rec] - start, take) + np.arange(int(take.sum()))
    return um[src], np.add.reduceat(take, first).astype(np.uint32)


def reference(off, lens, opts, v, mask, snaplen, ts, flags=0, cut=False, um=None):
    """(the EPB bytes of xfg_pcapng_write_captured, the selected packets' block
    lengths).  cut: hand the writer the selected packets only, each already
    cut to snaplen with its length as orig_len (for the largest batch)."""
    import xfgpu as G
    heads, ends, complete, sel = CM.form(opts, v, mask)
    keep = sel if cut else complete
    h = heads[keep]
    e = h if flags & HEAD_ONLY else ends[keep]
    cs = np.concatenate([[0], np.cumsum(lens)])
    total = (cs[e + 1] - cs[h]).astype(np.uint32)
    data, flens = gather(umem() if um is None else um, off, lens, h, e, snaplen if cut else None)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ref.pcapng")
        G.pcapng_write_captured(path, None, data, np.cumsum(flens, dtype=np.uint64) - flens, flens,
                                v[h], mask, snaplen, orig_lens=total,
                                ts_ns=np.ascontiguousarray(ts[h], np.uint64))
        blob = np.fromfile(path, np.uint8)
    pre = len(M.preamble("xdp", snaplen))
    assert blob[:pre].tobytes() == M.preamble("xdp", snaplen)
    st = total[M.selected(v[h], mask)].astype(np.int64)
    cap = np.minimum(st, snaplen) if snaplen else st
    return blob[pre:], 52 + ((cap + 3) & ~3)


def run(G, f, r, v, mask, snaplen, with_ts=True, flags=0, room=None, ts0=0, cut=False, stream=None):
    """One call; checks the three counts and the whole output buffer.
    room: a number, or a function of the total (None: the total)."""
    n = r.n
    v = np.asarray(v, np.uint8)
    ts = r.ts if with_ts else np.full(n, ts0, np.uint64)
    want, L = reference(r.off, r.lens, r.opts, v, mask, snaplen, ts, flags, cut)
    ends = np.cumsum(L)
    total = int(ends[-1]) if len(L) else 0
    assert total == len(want)
    room = total if room is None else room(total) if callable(room) else room
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
            d_ts.upload(r.ts)
        f.sync()
        f.capture_frags_into(r.batch, d_v.ptr, mask, d_out.ptr, room, d_c.ptr, snaplen=snaplen,
                             ts_ns_ptr=d_ts.ptr if with_ts else None, ts0=ts0, flags=flags,
                             stream=stream)
        f.sync()
        counts = d_c.download(np.zeros(3, np.uint64)).tolist()
        got = d_out.download(np.zeros(size, np.uint8))
    finally:
        for b in (d_out, d_c, d_v, d_ts):
            if b:
                b.free()
    print(f"n {n} selected {len(L)} total {total} room {room} flags {flags} counts {counts}")
    assert counts == [written, nbytes, len(L) - written]
    expect = np.full(size, A5, np.uint8)
    expect[:nbytes] = want[:nbytes]
    assert np.array_equal(got, expect), first_difference(got, expect)
    return got[:nbytes]


def both(G, f, r, v, mask, snaplen, **kw):
    """Whole packets, then XFG_CAPTURE_HEAD_ONLY on the same batch."""
    run(G, f, r, v, mask, snaplen, **kw)
    run(G, f, r, v, mask, snaplen, flags=HEAD_ONLY, **kw)


# ---- 1: record counts, as an array and as a ring
@pytest.mark.parametrize("ring", [False, True], ids=["array", "ring"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(G, filt, d_um, n, ring):
    k = SIZES.index(n)
    r, rng = make(G, filt, d_um, n, 100 + n, ring)
    try:
        both(G, filt, r, verdict_bytes(rng, r.opts & CONTD), MASK_DROP, SNAPS[k % len(SNAPS)],
             with_ts=k % 2 == 0, ts0=0x1122334455667788)
    finally:
        r.free()


# ---- 2: joins
def test_every_length_one(G, filt, d_um):
    """An output dword takes four records (five where the packet is longer)."""
    n = 3 * T + 7
    r, rng = make(G, filt, d_um, n, 7, lens=np.ones(n, np.int64))
    try:
        for snaplen in (0, 3):
            both(G, filt, r, verdict_bytes(rng, r.opts & CONTD), MASK_AD, snaplen)
    finally:
        r.free()


def test_every_length_zero_but_the_last(G, filt, d_um):
    n = T + 70
    rng = np.random.default_rng(8)
    cont = shapes(rng, n)
    cont[100:400] = 1                    # and one packet of 301 records
    cont[400] = 0
    cont[-1] = 0
    lens = np.where(cont == 0, LENSET[rng.integers(0, len(LENSET), n)], 0)
    r, rng = make(G, filt, d_um, n, 9, lens=lens, cont=cont)
    try:
        both(G, filt, r, verdict_bytes(rng, cont, frac=0.8), MASK_DROP, 0)
    finally:
        r.free()


def straddling(n, spans, seed):
    """Random shapes with one packet over each of the index ranges."""
    cont = shapes(np.random.default_rng(seed), n)
    for a, b in spans:
        cont[a - 1] = 0
        cont[a:b] = 1
        cont[b] = 0
    return cont


@pytest.mark.parametrize("spans", [[(62, 66), (254, 258), (T - 2, T + 2)], [(T - 1, 2 * T)]],
                         ids=["wave_pass_tile", "both_ends_of_a_tile"])
def test_packets_over_boundaries(G, filt, d_um, spans):
    n = 3 * T + 7
    cont = straddling(n, spans, 21)
    r, rng = make(G, filt, d_um, n, 22 + len(spans), ring=True, cont=cont)
    v = verdict_bytes(rng, cont)
    v[[a for a, _ in spans]] = DROP
    try:
        for snaplen in (0, 1514):
            both(G, filt, r, v, MASK_DROP, snaplen)
    finally:
        r.free()


@pytest.mark.parametrize("snaplen", [0, 96])
def test_a_long_packet(G, filt, d_um, snaplen):
    """One packet of 2T + 5 records, lengths 1..16, with packets on both sides."""
    side, k = 70, 2 * T + 5
    n = side + k + side
    rng = np.random.default_rng(31)
    cont = shapes(rng, n)
    cont[side - 1] = 0
    cont[side:side + k - 1] = 1
    cont[side + k - 1] = 0
    cont[-1] = 0
    lens = LENSET[rng.integers(0, len(LENSET), n)]
    lens[side:side + k] = rng.integers(1, 17, k)
    r, rng = make(G, filt, d_um, n, 32, lens=lens, cont=cont)
    v = verdict_bytes(rng, cont, frac=0.7)
    v[side] = DROP
    try:
        both(G, filt, r, v, MASK_DROP, snaplen)
    finally:
        r.free()


# ---- 3: snap lengths
@pytest.mark.parametrize("snaplen", SNAPS)
def test_snaplens(G, filt, d_um, snaplen):
    """Random packets behind two written by hand: records of 64, 1 and 200
    bytes (60 cuts the head, 64 and 65 fall on its joins, 96 cuts the third
    record) and of 1000, 514 and 2048 (1514 on a join, 4000 past the end)."""
    n = 3 * T + 7
    rng = np.random.default_rng(41)
    cont = shapes(rng, n)
    cont[:7] = [1, 1, 0, 1, 1, 0, 0]
    lens = LENSET[rng.integers(0, len(LENSET), n)]
    lens[:6] = [64, 1, 200, 1000, 514, 2048]
    r, rng = make(G, filt, d_um, n, 42, lens=lens, cont=cont)
    assert r.lens[:6].tolist() == [64, 1, 200, 1000, 514, 2048 - 16]   # (what the headroom leaves)
    v = verdict_bytes(rng, cont)
    v[[0, 3]] = DROP
    try:
        both(G, filt, r, v, MASK_DROP, snaplen, with_ts=SNAPS.index(snaplen) % 2 == 1, ts0=5)
    finally:
        r.free()


# ---- 4: every record a packet of its own: xfg_capture_descs
@pytest.mark.parametrize("n", [65, 3 * T + 7])
def test_single_records_equal_capture_descs(G, filt, d_um, n):
    r, rng = make(G, filt, d_um, n, 50 + n, ring=True, cont=np.zeros(n, np.uint32))
    v = BYTES[rng.integers(0, len(BYTES), n)]
    v[rng.random(n) < 0.5] = DROP
    assert NONE not in v
    room = 1 << 23
    d_v, d_ts = filt.alloc(max(n, 16)), filt.alloc(8 * n)
    outs = [filt.alloc(room + GUARD), filt.alloc(room + GUARD)]
    cs = [filt.alloc(32), filt.alloc(32)]
    try:
        d_v.upload(v)
        d_ts.upload(r.ts)
        for snaplen in (0, 65):
            for o, c in zip(outs, cs):
                o.upload(np.full(room + GUARD, A5, np.uint8))
                c.upload(np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64))
            filt.sync()
            filt.capture_into(r.batch, d_v.ptr, MASK_AD, outs[0].ptr, room, cs[0].ptr,
                              snaplen=snaplen, ts_ns_ptr=d_ts.ptr)
            filt.capture_frags_into(r.batch, d_v.ptr, MASK_AD, outs[1].ptr, room, cs[1].ptr,
                                    snaplen=snaplen, ts_ns_ptr=d_ts.ptr)
            filt.sync()
            want_c, got_c = (c.download(np.zeros(3, np.uint64)).tolist() for c in cs)
            want, got = (o.download(np.zeros(room + GUARD, np.uint8)) for o in outs)
            assert got_c == want_c and want_c[0] == np.count_nonzero(M.selected(v, MASK_AD))
            assert np.array_equal(got, want), first_difference(got, want)
    finally:
        for b in [d_v, d_ts] + outs + cs:
            b.free()
        r.free()


# ---- 5: masks and verdict bytes
@pytest.mark.parametrize("mask", [MASK_DROP, MASK_AD, 1 << 4 | 1 << 31, M.MASK_ALL])
def test_masks(G, filt, d_um, mask):
    """Bit a selects the packets whose head's byte is a; 32 and 254 are live
    and never selected; the bytes of the other records select nothing."""
    n = 3 * T + 7
    r, rng = make(G, filt, d_um, n, 61)
    v = verdict_bytes(rng, r.opts & CONTD, frac=0.2)
    heads, _, complete, sel = CM.form(r.opts, v, M.MASK_ALL)
    assert set(np.unique(v[heads[sel]])) == {0, 1, 2, 3, 4, 31}
    assert {32, 254} <= set(np.unique(v[heads[complete & ~sel]]))
    try:
        both(G, filt, r, v, mask, 96)
    finally:
        r.free()


def test_none_bytes(G, filt, d_um):
    """XFG_VERDICT_NONE bytes as in the model's hand-written rows, over three
    tiles: between two runs, behind a run that ends in CONTD, inside a run
    (at a tile's edge too), and the batch ends in CONTD."""
    n = 3 * T + 7
    r, rng = make(G, filt, d_um, n, 71, ring=True)
    cont = (r.opts & CONTD).copy()
    v = verdict_bytes(rng, cont, frac=0.7)
    v[rng.random(n) < 0.03] = NONE               # anywhere: heads, middles, ends
    for at in (65, T - 1, T, 2 * T + 1):         # inside a run of five
        r.opts[at - 2:at + 2] |= CONTD
        r.opts[at + 2] &= ~np.uint32(CONTD)
        v[at - 2:at + 3] = DROP
        v[at] = NONE
    r.opts[300:303] |= CONTD                     # a run that ends in CONTD before a NONE record
    v[300:303], v[303] = DROP, NONE
    r.opts[-2:] |= CONTD                         # ... and at the end of the batch
    v[-2:] = DROP
    r.free()
    r = Recs(G, filt, d_um, r.off // CHUNK, r.off % CHUNK, r.lens, r.opts, r.ts, ring=True)
    _, _, complete, _ = CM.form(r.opts, v)
    assert 20 < np.count_nonzero(~complete)
    try:
        both(G, filt, r, v, MASK_AD, 64)
        both(G, filt, r, np.full(n, NONE, np.uint8), M.MASK_ALL, 0)
    finally:
        r.free()


# ---- 6: overflow
ROOMS = {"0": 0, "51": 51, "total-1": lambda t: t - 1, "total": lambda t: t,
         "total+16": lambda t: t + 16, "half": lambda t: t // 2 + 3}


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("n", [65, 3 * T + 7])
def test_overflow_writes_a_prefix(G, filt, d_um, n, room):
    r, rng = make(G, filt, d_um, n, 80 + n, ring=n == 65)
    try:
        both(G, filt, r, verdict_bytes(rng, r.opts & CONTD), MASK_AD, 65 if n == 65 else 0,
             room=ROOMS[room])
    finally:
        r.free()


def test_overflow_does_not_slip_a_smaller_packet_in(G, filt, d_um):
    """Packets of 3, 5 and 1 records: room for the first block and 60 bytes;
    the second block does not fit, the third (56 bytes) would."""
    cont = [1, 1, 0, 1, 1, 1, 1, 0, 0]
    lens = [20, 1, 43, 500, 0, 500, 7, 507, 1]
    r, _ = make(G, filt, d_um, 9, 90, lens=lens, cont=cont)
    try:
        got = run(G, filt, r, np.full(9, DROP, np.uint8), MASK_DROP, 0, with_ts=False, room=116 + 60)
        assert len(got) == 116
    finally:
        r.free()


# ---- 7: more tiles than workgroups
def test_every_workgroup_loops(G, filt, d_um):
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert (BIG + T - 1) // T > 4 * ncu
    r, rng = make(G, filt, d_um, BIG, 95)
    try:
        run(G, filt, r, verdict_bytes(rng, r.opts & CONTD, frac=0.1), MASK_DROP, 1, cut=True)
    finally:
        r.free()


# ---- 8: behind the classify calls
STRIDE = 160


@pytest.fixture(scope="module")
def classified(G):
    """The rule set and the 4,097 fuzz frames of test_gpu_capture.py's
    fixture in a UMEM, and a context with the rules loaded."""
    from test_gpu_descs import umem_of
    rules, pool = X.random_rules(77, n4=200, n6=80, ne=24, nports=40)
    data, lens = X.gen_fuzz(31, 4097, STRIDE, rules, pool)
    um, addr = umem_of(data, lens, STRIDE, seed=5)
    f = G.Filter(X.VARIANT_FEATURES["xdpfilt_dny_all"], ndev=1, descs_min_packets=1)
    f.load_rules(rules)
    d_u = f.alloc(um.nbytes + 64)
    d_u.upload(um)
    yield f, rules, um, addr, lens, d_u
    d_u.free()
    f.close()


def offsets_of(addr):
    return ((addr & np.uint64(2**48 - 1)) + (addr >> np.uint64(48))).astype(np.int64)


def with_continuations(rng, addr, lens, last_open):
    """Every frame a head followed by 0-3 continuation records (other frames'
    chunks, any length).  Returns (addr, lens, cont) of the records."""
    nh = len(lens)
    k = rng.integers(0, 4, nh)
    first = np.cumsum(k + 1) - (k + 1)
    n = int((k + 1).sum())
    is_head = np.zeros(n, bool)
    is_head[first] = True
    pick = rng.integers(0, nh, n)
    a = addr[pick]
    ln = rng.integers(0, STRIDE + 1, n).astype(np.int64)
    a[first], ln[first] = addr, lens
    cont = np.ones(n, np.uint32)
    cont[first + k] = 0
    if last_open:
        cont[-1] = 1
    return a, ln, cont


@pytest.mark.parametrize("where", ["library_stream", "caller_stream"])
def test_classify_descs_frags_then_capture(G, classified, where):
    import torch
    f, rules, um, addr, lens, d_u = classified
    rng = np.random.default_rng(3)
    a, ln, cont = with_continuations(rng, addr, lens, last_open=True)
    n, opts = len(ln), with_bits(cont)
    entries, first = 16384, 0xfffffff0
    assert n <= entries
    rec = np.full((entries, 2), 0xFFFFFFFFFFFFFFFF, np.uint64)
    slot = ((first + np.arange(n, dtype=np.uint64)) & np.uint64(0xffffffff)
            & np.uint64(entries - 1)).astype(np.int64)
    rec[slot, 0], rec[slot, 1] = a, ln.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    stream = torch.cuda.Stream() if where == "caller_stream" else None
    sp = stream.cuda_stream if stream else None
    room = 1 << 22
    d_rx, d_v, d_out, d_c = f.alloc(rec.nbytes), f.alloc(n), f.alloc(room), f.alloc(32)
    try:
        d_rx.upload(rec)
        d_v.upload(np.full(n, 0xA5, np.uint8))
        d_out.upload(np.full(room, A5, np.uint8))
        f.sync()
        before = state_of(G, f, rules)
        c3 = f.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=entries - 1,
                                    stream=sp)
        assert c3[0] == len(lens) - 1 and c3[1] + c3[2] == n and c3[2] > 0
        b = G.DescBatch(d_u.ptr, d_rx.ptr, first, entries - 1, c3[1])
        f.capture_frags_into(b, d_v.ptr, MASK_AD, d_out.ptr, room, d_c.ptr, snaplen=96, ts0=42,
                             stream=sp)
        if stream:
            stream.synchronize()
        f.sync()
        done = c3[1]
        v = d_v.download(np.zeros(n, np.uint8))[:done]
        assert 0 < np.count_nonzero(v == DROP) < done
        want, L = reference(offsets_of(a)[:done], ln[:done], opts[:done], v, MASK_AD, 96,
                            np.full(done, 42, np.uint64), um=um)
        assert d_c.download(np.zeros(3, np.uint64)).tolist() == [len(L), len(want), 0]
        expect = np.full(room, A5, np.uint8)
        expect[:len(want)] = want
        got = d_out.download(np.zeros(room, np.uint8))
        assert np.array_equal(got, expect), first_difference(got, expect)
        # the capture is inert: a second one changes no map value and no statistic
        after_classify = state_of(G, f, rules)
        f.capture_frags_into(b, d_v.ptr, M.MASK_ALL, d_out.ptr, room, d_c.ptr, stream=sp)
        f.sync()
        for x, y in zip(after_classify, state_of(G, f, rules)):
            np.testing.assert_array_equal(x, y)
        assert any(not np.array_equal(x, y) for x, y in zip(before, after_classify))
    finally:
        for buf in (d_rx, d_v, d_out, d_c):
            buf.free()


def socket_counts(nsocks):
    if nsocks == 1:
        return [T + 77]
    if nsocks == 3:
        return [T + 5, 40, 300]
    k = np.random.default_rng(64).integers(0, 40, nsocks)
    k[[0, 7, 8, 63]] = 0
    return [int(x) for x in k]


@pytest.mark.parametrize("nsocks", [1, 3, 64])
def test_classify_socks_frags_then_capture(G, classified, nsocks):
    """The capture over sk->flat with the call's verdicts equals the
    per-socket references over each socket's first done[s] records, in socket
    order.  Some sockets are empty, some have no end-of-packet record, some
    end in an incomplete packet whose last record has CONTD set and is
    followed by the next socket's head."""
    f, rules, um, addr, lens, d_u = classified
    counts = socket_counts(nsocks)
    base = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(base[-1])
    rng = np.random.default_rng(200 + nsocks)
    pick = rng.integers(0, len(lens), n)
    a, ln = addr[pick], lens[pick].astype(np.int64)
    cont = shapes(rng, n)
    open_end, no_eop = [], []
    for s in range(nsocks):
        lo, hi = int(base[s]), int(base[s + 1])
        if hi == lo:
            continue
        if s % 4 == 1 and nsocks > 1:
            cont[lo:hi] = 1
            no_eop.append(s)
        elif s % 2 == 0:
            cont[hi - 1] = 1             # ends inside a packet, the next socket's head behind it
            open_end.append(s)
        else:
            cont[hi - 1] = 0
    assert open_end and (nsocks == 1 or no_eop)
    opts = with_bits(cont)
    rec = np.stack([a, ln.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))], axis=1)
    room = 1 << 22
    d_rx, d_flat, d_v = f.alloc(16 * n + 16), f.alloc(16 * n), f.alloc(n)
    d_out, d_c = f.alloc(room), f.alloc(32)
    try:
        d_rx.upload(np.ascontiguousarray(rec))
        d_flat.upload(np.full((n, 2), 0xA5A5A5A5A5A5A5A5, np.uint64))
        d_v.upload(np.full(n, 0xA5, np.uint8))
        d_out.upload(np.full(room, A5, np.uint8))
        f.sync()
        socks = [dict(rx_descs=d_rx.ptr + 16 * int(base[s]), count=counts[s]) for s in range(nsocks)]
        done, c3 = f.classify_socks_frags(d_u.ptr, socks, d_v.ptr, flat_ptr=d_flat.ptr)
        b = G.DescBatch(d_u.ptr, d_flat.ptr, 0, 0xffffffff, n)
        f.capture_frags_into(b, d_v.ptr, MASK_AD, d_out.ptr, room, d_c.ptr, snaplen=0, ts0=7)
        f.sync()
        v = d_v.download(np.zeros(n, np.uint8))
        assert all(done[s] == 0 for s in no_eop) and all(done[s] < counts[s] for s in open_end)
        assert c3[2] > 0 and np.count_nonzero(v == NONE) == c3[2]
        off = offsets_of(a)
        parts, nblocks = [], 0
        for s in range(nsocks):
            lo, hi = int(base[s]), int(base[s]) + int(done[s])
            w, L = reference(off[lo:hi], ln[lo:hi], opts[lo:hi], v[lo:hi], MASK_AD, 0,
                             np.full(hi - lo, 7, np.uint64), um=um)
            parts.append(w)
            nblocks += len(L)
        want = np.concatenate(parts)
        assert nblocks > 0
        assert d_c.download(np.zeros(3, np.uint64)).tolist() == [nblocks, len(want), 0]
        expect = np.full(room, A5, np.uint8)
        expect[:len(want)] = want
        got = d_out.download(np.zeros(room, np.uint8))
        assert np.array_equal(got, expect), first_difference(got, expect)
    finally:
        for buf in (d_rx, d_flat, d_v, d_out, d_c):
            buf.free()


# ---- 9: the binding's convenience call, and a file built from its blocks
def test_capture_descs_frags_returns_blocks_written_lost(G, filt, d_um, tmp_path):
    n = T + 7
    r, rng = make(G, filt, d_um, n, 99)
    v = verdict_bytes(rng, r.opts & CONTD)
    d_v, d_ts = filt.alloc(n), filt.alloc(8 * n)
    d_v.upload(v)
    d_ts.upload(r.ts)
    try:
        want, L = reference(r.off, r.lens, r.opts, v, MASK_DROP, 60, r.ts)
        blocks, written, lost = filt.capture_descs_frags(r.batch, d_v.ptr, MASK_DROP, snaplen=60,
                                                         out_bytes=1 << 21, ts_ns=d_ts.ptr)
        assert (written, lost) == (len(L), 0) and blocks.dtype == np.uint8
        assert np.array_equal(blocks, want)
        few, written, lost = filt.capture_descs_frags(r.batch, d_v.ptr, MASK_DROP, snaplen=60,
                                                      out_bytes=int(L[:10].sum()) + 50,
                                                      ts_ns=d_ts.ptr)
        assert (written, lost) == (10, len(L) - 10)
        assert np.array_equal(few, want[:int(L[:10].sum())])
        heads, ends, _, sel = CM.form(r.opts, v, MASK_DROP)
        cs = np.concatenate([[0], np.cumsum(r.lens)])
        total = cs[ends[sel] + 1] - cs[heads[sel]]
        path = tmp_path / "dev.pcapng"
        G.pcapng_begin(path, "veth0", 60)
        G.pcapng_append(path, blocks)
        rdata, roffs, rlens, rorig, rts = G.read_pcap(path)
        assert rlens.tolist() == np.minimum(total, 60).tolist()
        assert rorig.tolist() == total.tolist() and rts.tolist() == r.ts[heads[sel]].tolist()
        assert total.max() > 60 and len(total) > 100
    finally:
        r.free()
        d_v.free()
        d_ts.free()

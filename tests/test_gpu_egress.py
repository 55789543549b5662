"""AF_XDP egress (xfg_ring_egress, xfg_egress.hip): TX records of the PASS
frames and fill addresses of every other frame of an RX descriptor batch.

The model is a few lines of numpy over the same arrays -- the mask v == 2,
addr[mask] and len[mask] for the TX ring, addr[~mask] & (2^48 - 1) for the
fill ring -- and every comparison is exact.  Each output ring is compared
whole against a copy of what was uploaded (0xA5 bytes) with the expected
entries written in, so entries outside the written ranges, and those past
counts[0] / counts[1] inside the reserved ranges, must come back untouched.
"""
import functools
import os
import re

import numpy as np
import pytest

import xftools as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS = 2
OTHERS = np.array([0, 1, 3, 4, 255], np.uint8)     # every verdict byte but PASS counts as "other"
ADDR48 = np.uint64(2**48 - 1)
A5 = np.uint64(0xA5A5A5A5A5A5A5A5)
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 7,
         3 * 65536 + 7, 2**22 + 13]
PATTERNS = ["random", "all_pass", "no_pass", "alternating", "tile_last"]


def tile():
    src = open(os.path.join(ROOT, "xdp-tools_amd", "csrc", "xfg_layout.h")).read()
    return int(re.search(r"#define\s+XFG_EGRESS_TILE\s+(\d+)u", src).group(1))


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
def batch_of(n):
    """addr, len and options of n RX records (read only): chunks of 4 KiB in
    permuted order at headroom 0 / 16 / 256, every third address in the
    unaligned-chunk form (offset in bits 48..63); some records carry option
    bits, which a TX record must not."""
    rng = np.random.default_rng(1000 + n)
    i = np.arange(n)
    base = rng.permutation(n + 7)[:n].astype(np.uint64) * np.uint64(4096)
    head = np.choose(i % 3, [0, 256, 16]).astype(np.uint64)
    addr = np.where(i % 3 == 2, base | (head << np.uint64(48)), base + head).astype(np.uint64)
    lens = rng.integers(14, 1515, n).astype(np.uint32)
    opts = np.where(i % 5 == 4, 1 << 16, 0).astype(np.uint32)
    for a in (addr, lens, opts):
        a.setflags(write=False)
    return addr, lens, opts


@functools.lru_cache(maxsize=None)
def verdicts_of(n, pattern):
    rng = np.random.default_rng(8 * n + PATTERNS.index(pattern))
    v = OTHERS[rng.integers(0, len(OTHERS), n)]      # 3 and 255 among them
    if pattern == "random":
        v[rng.random(n) < 0.5] = PASS
    elif pattern == "all_pass":
        v[:] = PASS
    elif pattern == "alternating":
        v[0::2] = PASS
    elif pattern == "tile_last":
        v[tile() - 1::tile()] = PASS
    other = np.flatnonzero(v != PASS)
    if len(other) >= 2:                              # ... whatever the draw
        v[other[0]], v[other[-1]] = 3, 255
    v.setflags(write=False)
    return v


def records(addr, lens, opts):
    r = np.empty((len(addr), 2), np.uint64)
    r[:, 0] = addr
    r[:, 1] = lens.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    return r


def slots(first, count, mask):
    """Ring slots of entries first .. first + count - 1 (the u32 index wraps)."""
    return ((first + np.arange(count, dtype=np.uint64)) & np.uint64(0xffffffff)
            & np.uint64(mask)).astype(np.int64)


def pow2_at_least(n):
    e = 16
    while e < n:
        e *= 2
    return e


class Rings:
    """The three rings of a case: a plain array each (a few entries to
    spare), or power-of-two rings with their firsts chosen apart."""

    def __init__(self, n, kind, rot=0):
        if kind == "array":
            self.entries = (n + 5, n + 5, n + 5)
            self.first = (0, 0, 0)
            self.mask = (0xffffffff,) * 3
        else:
            # rx and tx at exactly the batch's size, fill twice it; one first
            # is 0xfffffff0 (the u32 index itself wraps 16 entries in), one
            # wraps its ring mid-batch, one does and lies past the mask
            e = pow2_at_least(n)
            self.entries = (e, e, 2 * e)
            how = ["u32", "mid", "past"]
            how = how[rot % 3:] + how[:rot % 3]
            self.first = tuple({"u32": 0xfffffff0, "mid": en - (n // 4 + 1),
                                "past": 4 * en - (n // 3 + 1)}[h] for h, en in zip(how, self.entries))
            self.mask = tuple(en - 1 for en in self.entries)
            if n > 16:      # every ring wraps inside what half the batch writes
                for fi, en in zip(self.first, self.entries):
                    assert fi < 2**32 and (fi == 0xfffffff0 or (fi & (en - 1)) + n // 2 > en)


def model(addr, lens, v):
    m = v == PASS
    tx = np.empty((int(m.sum()), 2), np.uint64)
    tx[:, 0] = addr[m]
    tx[:, 1] = lens[m].astype(np.uint64)             # options 0
    return tx, addr[~m] & ADDR48


def run_egress(f, n, v, rings, tx=True, fill=True, umem=None, flags=0, stream=None, batch=None):
    """One call over batch_of(n) (or @batch); checks counts, both rings whole,
    and returns the downloaded UMEM (when there is one)."""
    addr, lens, opts = batch or batch_of(n)
    rx_e, tx_e, fill_e = rings.entries
    rx_h = np.full((max(rx_e, 1), 2), A5, np.uint64)
    rx_h[slots(rings.first[0], n, rings.mask[0])] = records(addr, lens, opts)
    tx_h = np.full((max(tx_e, 1), 2), A5, np.uint64)
    fill_h = np.full(max(fill_e, 1), A5, np.uint64)
    d_rx, d_tx, d_fill = f.alloc(rx_h.nbytes), f.alloc(tx_h.nbytes), f.alloc(fill_h.nbytes)
    d_v, d_c = f.alloc(max(n, 16)), f.alloc(16)
    d_u = None
    bufs = [d_rx, d_tx, d_fill, d_v, d_c]
    try:
        d_rx.upload(rx_h)
        d_tx.upload(tx_h)
        d_fill.upload(fill_h)
        d_c.upload(np.full(2, A5, np.uint64))
        if n and v is not None:
            d_v.upload(v)
        if umem is not None:
            d_u = f.alloc(umem.nbytes)
            bufs.append(d_u)
            d_u.upload(umem)
        f.ring_egress(d_rx.ptr, n, d_v.ptr if v is not None else None, d_c.ptr,
                      tx_ptr=d_tx.ptr if tx else None, fill_ptr=d_fill.ptr if fill else None,
                      rx_first=rings.first[0], rx_mask=rings.mask[0],
                      tx_first=rings.first[1], tx_mask=rings.mask[1],
                      fill_first=rings.first[2], fill_mask=rings.mask[2],
                      umem_ptr=d_u.ptr if d_u else None, flags=flags, stream=stream)
        f.sync()
        counts = d_c.download(np.zeros(2, np.uint64))
        got_tx = d_tx.download(np.zeros_like(tx_h))
        got_fill = d_fill.download(np.zeros_like(fill_h))
        got_umem = d_u.download(np.zeros_like(umem)) if d_u else None
    finally:
        for b in bufs:
            b.free()
    vv = v if tx else np.zeros(n, np.uint8)           # no TX ring: every frame is "other"
    want_tx, want_fill = model(addr, lens, vv)
    assert counts.tolist() == [len(want_tx), len(want_fill)]
    assert len(want_tx) + len(want_fill) == n
    if tx:
        tx_h[slots(rings.first[1], len(want_tx), rings.mask[1])] = want_tx
    if fill:
        fill_h[slots(rings.first[2], len(want_fill), rings.mask[2])] = want_fill
    np.testing.assert_array_equal(got_tx, tx_h)
    np.testing.assert_array_equal(got_fill, fill_h)
    return got_umem


# ---- 1: sizes x verdict patterns x ring forms
@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_partition(filt, n, pattern, kind):
    if n == SIZES[-1]:   # workgroups take more than one tile only past 4 tiles a CU
        import torch
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        assert (n + tile() - 1) // tile() > 4 * ncu
    run_egress(filt, n, verdicts_of(n, pattern), Rings(n, kind, rot=PATTERNS.index(pattern)))


# ---- 2: the degenerate shapes
@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("n", [0, 1, 257, 4097, 3 * 65536 + 7])
def test_no_tx_ring_is_rx_drop(filt, n, kind):
    """tx == NULL: every chunk to the fill ring, verdicts not read (NULL)."""
    run_egress(filt, n, None, Rings(n, kind), tx=False)
    # (nor read when given: an all-PASS buffer changes nothing)
    run_egress(filt, n, verdicts_of(n, "all_pass"), Rings(n, kind, rot=1), tx=False)


@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("pattern", ["random", "no_pass"])
@pytest.mark.parametrize("n", [1, 257, 4097, 3 * 65536 + 7])
def test_no_fill_ring(filt, n, pattern, kind):
    """fill == NULL: the TX ring alone; counts[1] still counts the rest."""
    run_egress(filt, n, verdicts_of(n, pattern), Rings(n, kind, rot=2), fill=False)


# ---- 3: the MAC swap
def umem_for(n, chunk=64):
    """A UMEM of random bytes and n descriptors naming distinct frames in it
    (headroom 0 / 16 / 32, every third address in the offset form)."""
    rng = np.random.default_rng(50 + n)
    nchunks = n + 7
    umem = rng.integers(0, 256, nchunks * chunk, dtype=np.uint8)
    i = np.arange(n)
    base = rng.permutation(nchunks)[:n].astype(np.uint64) * np.uint64(chunk)
    head = (16 * (i % 3)).astype(np.uint64)
    addr = np.where(i % 3 == 2, base | (head << np.uint64(48)), base + head).astype(np.uint64)
    return umem, addr, (base + head).astype(np.int64)


@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("pattern", ["random", "all_pass", "no_pass"])
@pytest.mark.parametrize("n", [1, 65, 4097, 3 * 65536 + 7])
def test_swap_macs(G, filt, n, pattern, kind):
    umem, addr, start = umem_for(n)
    _, lens, opts = batch_of(n)
    batch = (addr, lens, opts)
    v = verdicts_of(n, pattern)
    got = run_egress(filt, n, v, Rings(n, kind), umem=umem, flags=G.EGRESS_SWAP_MACS, batch=batch)
    want = umem.copy()
    at = start[v == PASS][:, None] + np.arange(12)
    want[at] = umem[at][:, [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]]
    # bytes 12.. of the PASS frames, every other frame and the spare chunks:
    # identical (the whole UMEM is compared)
    np.testing.assert_array_equal(got, want)
    # without a TX ring there is no PASS frame to swap
    got = run_egress(filt, n, None, Rings(n, kind), tx=False, umem=umem, flags=G.EGRESS_SWAP_MACS,
                     batch=batch)
    np.testing.assert_array_equal(got, umem)


# ---- 4: stream order after classify_descs
STRIDE, CHUNK = 160, 256


@pytest.fixture(scope="module")
def classified(G):
    """A small mixed rule set, 4,097 fuzz frames in a UMEM, the oracle's
    verdicts, and a context with the rules loaded."""
    from test_gpu_descs import ring_of, umem_of
    rules, pool = X.random_rules(77, n4=200, n6=80, ne=24, nports=40)
    data, lens = X.gen_fuzz(31, 4097, STRIDE, rules, pool)
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    ov, _, _ = X.run_oracle(feats, data, lens, rules, stride=STRIDE)
    assert 0 < np.count_nonzero(ov == PASS) < len(ov)
    umem, addr = umem_of(data, lens, STRIDE, seed=5)
    descs, first, mask = ring_of(addr, lens, 8192, 8192 - 777, fill=0xFF)
    f = G.Filter(feats, ndev=1, descs_min_packets=1)
    f.load_rules(rules)
    yield f, umem, addr, lens, descs, first, mask, ov
    f.close()


@pytest.mark.parametrize("where", ["library_stream", "caller_stream"])
def test_classify_then_egress_without_sync(G, classified, where):
    import torch
    f, umem, addr, lens, descs, first, mask, ov = classified
    n = len(lens)
    stream = torch.cuda.Stream() if where == "caller_stream" else None
    sp = stream.cuda_stream if stream else None
    tx_h = np.full((8192, 2), A5, np.uint64)
    fill_h = np.full(8192, A5, np.uint64)
    d_u, d_rx, d_v = f.alloc(umem.nbytes), f.alloc(descs.nbytes), f.alloc(n)
    d_tx, d_fill, d_c = f.alloc(tx_h.nbytes), f.alloc(fill_h.nbytes), f.alloc(16)
    d_u.upload(umem)
    d_rx.upload(descs)
    d_v.upload(np.zeros(n, np.uint8))
    d_tx.upload(tx_h)
    d_fill.upload(fill_h)
    f.sync()
    f.classify_descs(d_u.ptr, d_rx.ptr, n, d_v.ptr, first=first, mask=mask, stream=sp)
    f.ring_egress(d_rx.ptr, n, d_v.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                  rx_first=first, rx_mask=mask, tx_first=8192 - 100, tx_mask=8191,
                  fill_first=0xfffffff0, fill_mask=8191, stream=sp)
    if stream:
        stream.synchronize()
    f.sync()
    assert f.last_path() == G.Filter.PATH_PIPELINE
    np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), ov)
    want_tx, want_fill = model(addr, lens, ov)
    assert d_c.download(np.zeros(2, np.uint64)).tolist() == [len(want_tx), len(want_fill)]
    tx_h[slots(8192 - 100, len(want_tx), 8191)] = want_tx
    fill_h[slots(0xfffffff0, len(want_fill), 8191)] = want_fill
    np.testing.assert_array_equal(d_tx.download(np.zeros_like(tx_h)), tx_h)
    np.testing.assert_array_equal(d_fill.download(np.zeros_like(fill_h)), fill_h)
    for b in (d_u, d_rx, d_v, d_tx, d_fill, d_c):
        b.free()


# ---- 5: the status words shared with xfg_compact
@pytest.mark.parametrize("where", ["library_stream", "caller_stream"])
def test_scratch_shared_with_compact(filt, where):
    """compact, ring_egress, compact, ring_egress back to back without a
    sync, of sizes whose tile counts differ both ways: each launch finds the
    other kernel's status words and ticket where its own go."""
    import torch
    f = filt
    stream = torch.cuda.Stream() if where == "caller_stream" else None
    sp = stream.cuda_stream if stream else None
    sizes = [3 * 65536 + 7, 100003, 50001, 2**18 + 1]      # compact, egress, compact, egress
    held, jobs = [], []
    for k, n in enumerate(sizes):
        v = verdicts_of(n, "random")
        d_v, d_c = f.alloc(n), f.alloc(16)
        d_v.upload(v)
        d_c.upload(np.full(2, A5, np.uint64))
        held += [d_v, d_c]
        if k % 2 == 0:
            d_i = f.alloc(4 * n)
            held.append(d_i)
            jobs.append(("compact", n, v, d_v, d_c, d_i))
        else:
            addr, lens, opts = batch_of(n)
            d_rx, d_tx, d_fill = f.alloc(16 * n), f.alloc(16 * n), f.alloc(8 * n)
            d_rx.upload(records(addr, lens, opts))
            held += [d_rx, d_tx, d_fill]
            jobs.append(("egress", n, v, d_v, d_c, d_rx, d_tx, d_fill))
    f.sync()
    for job in jobs:
        if job[0] == "compact":
            _, n, v, d_v, d_c, d_i = job
            f.compact(d_v.ptr, n, PASS, d_i.ptr, d_c.ptr, stream=sp)
        else:
            _, n, v, d_v, d_c, d_rx, d_tx, d_fill = job
            f.ring_egress(d_rx.ptr, n, d_v.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                          stream=sp)
    if stream:
        stream.synchronize()
    f.sync()
    for job in jobs:
        if job[0] == "compact":
            _, n, v, d_v, d_c, d_i = job
            want = np.flatnonzero(v == PASS).astype(np.uint32)
            assert int(d_c.download(np.zeros(1, np.uint64))[0]) == len(want)
            np.testing.assert_array_equal(d_i.download(np.zeros(len(want), np.uint32)), want)
        else:
            _, n, v, d_v, d_c, d_rx, d_tx, d_fill = job
            addr, lens, _ = batch_of(n)
            want_tx, want_fill = model(addr, lens, v)
            assert d_c.download(np.zeros(2, np.uint64)).tolist() == [len(want_tx), len(want_fill)]
            np.testing.assert_array_equal(d_tx.download(np.zeros_like(want_tx)), want_tx)
            np.testing.assert_array_equal(d_fill.download(np.zeros_like(want_fill)), want_fill)
    for b in held:
        b.free()

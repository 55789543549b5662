"""AF_XDP descriptor batches (xfg_classify_descs) on the generic pipelined
kernel's descriptor mode (xfg_pipeline.hip, SRC_DESCS).

Every comparison is against the CPU oracle over the same frames: verdicts,
stats, every IPv4 / IPv6 / Ethernet rule value and all 65,536 port values.
The frames live in a UMEM in device memory and are named by xdp_desc records
{u64 addr; u32 len; u32 options} in a ring (or a plain array).

By default a descriptor batch below XFG_DESCS_PIPE_MIN packets (2^16) keeps
the general kernel, whose fixed cost is lower; the tests open the context
with descs_min_packets=1 so that their small batches run the descriptor
mode (as the quotient-index tests open theirs with qt_min_keys=1), and the
path test checks the default routing on either side of the bound.
"""
import errno
import os
import re

import numpy as np
import pytest

import xftools as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 160          # gen_fuzz slot
CHUNK = 256           # UMEM chunk of the generated batches
ALL_PORTS = np.arange(65536, dtype=np.uint32)


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@pytest.fixture(scope="module")
def mixed():
    """The shared rule set and its fuzz frames (4,097 of them), read only."""
    rules, pool = X.random_rules(77, n4=200, n6=80, ne=24, nports=40)
    data, lens = X.gen_fuzz(31, 4097, STRIDE, rules, pool)
    return rules, pool, data, lens


def layout_const(name, file="xfg_layout.h"):
    src = open(os.path.join(ROOT, "xdp-tools_amd", "csrc", file)).read()
    m = re.search(r"#define\s+%s\s+\(?(\d+)u?(?:ll)?\s*(?:<<\s*(\d+))?" % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


def umem_of(data, lens, stride, seed, chunk=CHUNK, spare=7):
    """Frames of a fixed-stride batch into a UMEM of @chunk-byte chunks in
    permuted order, at headroom 0 / 16 / 32; every third address in the
    unaligned-chunk form (offset in bits 48..63).  Returns (umem, addr)."""
    n = len(lens)
    rng = np.random.default_rng(seed)
    nchunks = n + spare
    perm = rng.permutation(nchunks)[:n].astype(np.uint64)
    umem = np.zeros((nchunks, chunk), np.uint8)
    slots = data.reshape(n, stride)
    i = np.arange(n)
    head = (16 * (i % 3)).astype(np.uint64)
    assert int(head.max()) + stride <= chunk
    for h in (0, 16, 32):
        sel = head == h
        umem[perm[sel], h:h + stride] = slots[sel]
    base = perm * np.uint64(chunk)
    addr = np.where(i % 3 == 2, base | (head << np.uint64(48)), base + head)
    return umem.reshape(-1), addr.astype(np.uint64)


def ring_of(addr, lens, entries=None, first=0, fill=0):
    """xdp_desc records of the batch in a ring of @entries (None: a plain
    array, mask 0xffffffff) starting at @first; every byte of the entries
    outside the batch is @fill.  Returns (descs, first, mask)."""
    n = len(lens)
    if entries is None:
        descs = np.zeros((n, 2), np.uint64)
        descs[:, 0] = addr
        descs[:, 1] = lens.astype(np.uint64)
        return descs, 0, 0xffffffff
    assert n <= entries and entries & (entries - 1) == 0
    descs = np.full((entries, 2), fill * 0x0101010101010101, np.uint64)
    idx = (first + np.arange(n)) & (entries - 1)
    descs[idx, 0] = addr
    descs[idx, 1] = lens.astype(np.uint64)     # len | options 0 << 32
    return descs, first, entries - 1


class Dev:
    """A batch in device memory."""

    def __init__(self, f, umem, descs, n):
        self.f, self.n = f, n
        self.umem, self.descs, self.v = f.alloc(umem.nbytes), f.alloc(descs.nbytes), f.alloc(max(n, 1))
        self.umem.upload(umem)
        self.descs.upload(descs)

    def classify(self, first, mask):
        self.f.classify_descs(self.umem.ptr, self.descs.ptr, self.n, self.v.ptr, first=first, mask=mask)
        self.f.sync()
        return self.v.download(np.zeros(self.n, np.uint8))


def check_all(G, f, rules, ov, orules, ost, v=None):
    if v is not None:
        np.testing.assert_array_equal(v, ov)
    np.testing.assert_array_equal(f.stats(), ost)
    r = rules.prepared()
    np.testing.assert_array_equal(f.values_of(G.MAP_IPV4, r.v4_keys), orules.v4_vals)
    np.testing.assert_array_equal(f.values_of(G.MAP_IPV6, r.v6_keys), orules.v6_vals)
    np.testing.assert_array_equal(f.values_of(G.MAP_ETHERNET, r.eth_keys), orules.eth_vals)
    np.testing.assert_array_equal(f.values_of(G.MAP_PORTS, ALL_PORTS), orules.ports)


def run_case(G, feats, rules, data, lens, stride, entries, first, fill=0, want_path=None, **opts):
    opts.setdefault("descs_min_packets", 1)
    ov, orules, ost = X.run_oracle(feats, data, lens, rules, stride=stride)
    umem, addr = umem_of(data, lens, stride, seed=len(lens))
    descs, first, mask = ring_of(addr, lens, entries, first, fill)
    f = G.Filter(feats, ndev=1, **opts)
    f.load_rules(rules)
    v = Dev(f, umem, descs, len(lens)).classify(first, mask)
    if want_path is not None:
        assert f.last_path() == want_path
    check_all(G, f, rules, ov, orules, ost, v)
    f.close()


# ---- 1: the path
def test_descs_take_the_pipelined_kernel(G, mixed):
    rules, pool, data, lens = mixed
    all_, eth = X.VARIANT_FEATURES["xdpfilt_dny_all"], X.VARIANT_FEATURES["xdpfilt_dny_eth"]
    # a context opened with the defaults: from XFG_DESCS_PIPE_MIN packets
    bound = layout_const("XFG_DESCS_PIPE_MIN", "xfg_plan.h")
    bdata, blens = X.gen_fuzz(32, bound, STRIDE, rules, pool)
    run_case(G, all_, rules, bdata, blens, STRIDE, None, 0, want_path=G.Filter.PATH_PIPELINE,
             descs_min_packets=0)
    # the Ethernet-only programs keep the general kernel
    run_case(G, eth, rules, bdata, blens, STRIDE, None, 0, want_path=G.Filter.PATH_GENERAL,
             descs_min_packets=0)
    # below the bound the general kernel, unless the context lowers it
    n = 1000
    run_case(G, all_, rules, data[:n * STRIDE], lens[:n], STRIDE, None, 0,
             want_path=G.Filter.PATH_GENERAL, descs_min_packets=0)
    run_case(G, all_, rules, data[:n * STRIDE], lens[:n], STRIDE, None, 0,
             want_path=G.Filter.PATH_PIPELINE)
    run_case(G, eth, rules, data[:n * STRIDE], lens[:n], STRIDE, None, 0,
             want_path=G.Filter.PATH_GENERAL)


# ---- 2: all ten programs
@pytest.mark.parametrize("prog", [name for name, _ in X.VARIANTS])
def test_descs_every_program(G, mixed, prog):
    rules, _, data, lens = mixed
    eth = prog.endswith("_eth")
    run_case(G, X.VARIANT_FEATURES[prog], rules, data, lens, STRIDE, 8192, 8192 - 777,
             want_path=G.Filter.PATH_GENERAL if eth else G.Filter.PATH_PIPELINE)


# ---- 3: tile and wave edges; the ring outside the batch is 0xFF bytes
@pytest.mark.parametrize("ring", ["array", "wrap"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 1025])
def test_descs_tile_and_wave_edges(G, mixed, n, ring):
    rules, _, data, lens = mixed
    if ring == "array":
        entries, first = None, 0
    else:
        entries = 2048
        first = entries - (n // 2 + 1)     # the batch wraps
    run_case(G, X.VARIANT_FEATURES["xdpfilt_dny_all"], rules, data[:n * STRIDE], lens[:n], STRIDE,
             entries, first, fill=0xFF, want_path=G.Filter.PATH_PIPELINE)


# ---- 4: lengths
EDGE_LENS = [0, 1, 13, 14, 15, 16, 17, 33, 34, 47, 48, 49, 63, 64, 65]


def test_descs_lengths(G, mixed):
    """Short frames, frames in the UMEM's last bytes, and two frames longer
    than any 16-bit length.  The UMEM is a multiple of 16 bytes and no more:
    a frame of a length that is a multiple of 16 ends at its last byte, any
    other in its last 16 (frame starts are 16-byte aligned)."""
    rules, _, data, lens = mixed
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    slots = data.reshape(-1, STRIDE)
    full = np.flatnonzero(lens >= 74)      # frames to cut down
    rng = np.random.default_rng(8)
    big = [70000, 65535]
    parts, offs, ls = [], [], []
    pos = 0
    # the two long frames: a real header, then payload bytes
    for j, L in enumerate(big):
        fr = rng.integers(0, 256, (L + 15) & ~15, dtype=np.uint8)
        fr[:STRIDE] = slots[full[j]]
        parts.append(fr)
        offs.append(pos)
        ls.append(L)
        pos += len(fr)
    # every edge length at its own chunk (three different frames each)
    for j, L in enumerate(EDGE_LENS * 3):
        parts.append(slots[full[10 + j]][:80])
        offs.append(pos)
        ls.append(L)
        pos += 80
    # ... and in the last bytes of the UMEM: its last 80 bytes are one frame,
    # and a frame of length L starts at the last 16-byte boundary that holds it
    parts.append(slots[full[100]][:80])
    pos += 80
    for L in EDGE_LENS:
        offs.append(pos - ((L + 15) & ~15))
        ls.append(L)
    umem = np.concatenate(parts)
    assert umem.nbytes == pos and pos % 16 == 0
    ends = np.array(offs) + np.array(ls)
    assert np.count_nonzero(ends == pos) >= 4 and np.all(ends <= pos)
    offs, ls = np.array(offs, np.uint64), np.array(ls, np.uint32)
    n = len(ls)
    assert n <= 128
    order = rng.permutation(n)              # the long frames anywhere in the tiles
    offs, ls = offs[order], ls[order]
    ov, orules, ost = X.run_oracle(feats, umem, ls, rules, offsets=offs)
    assert int(ost[:, 1].sum()) == int(ls.sum())
    descs, first, mask = ring_of(offs, ls, 256, 256 - 50, fill=0xFF)
    f = G.Filter(feats, ndev=1, descs_min_packets=1)
    f.load_rules(rules)
    v = Dev(f, umem, descs, n).classify(first, mask)
    assert f.last_path() == G.Filter.PATH_PIPELINE
    check_all(G, f, rules, ov, orules, ost, v)
    f.close()


# ---- 5: windows
def be16(x):
    return [(x >> 8) & 0xff, x & 0xff]


def far_frames(rules, count, seed):
    """Frames whose parse reads past byte 64: IPv6/TCP (the data offset at
    byte 66), IPv4 with options + UDP, VLAN + IPv6 + two extension headers +
    UDP; some addressed to ruled keys.  Returns [count, STRIDE] slots, lens."""
    rng = np.random.default_rng(seed)
    r = rules.prepared()
    out = np.zeros((count, STRIDE), np.uint8)
    lens = np.zeros(count, np.uint32)
    for i in range(count):
        kind = i % 3
        mac = list(rng.integers(0, 256, 12))
        v6 = [list(rng.integers(0, 256, 16)), list(rng.integers(0, 256, 16))]
        v4 = [list(rng.integers(0, 256, 4)), list(rng.integers(0, 256, 4))]
        if i % 2 and len(r.v6_keys):
            v6[int(rng.integers(2))] = list(r.v6_keys[int(rng.integers(len(r.v6_keys)))])
        if i % 2 and len(r.v4_keys):
            v4[int(rng.integers(2))] = list(r.v4_keys[int(rng.integers(len(r.v4_keys)))])
        ports = be16(int(rng.integers(65536))) + be16(int(rng.integers(65536)))
        udp = ports + be16(8 + 12) + [0, 0] + [0xab] * 12
        tcp = ports + [0] * 8 + [0x50, 0x10] + [0] * 6 + [0xcd] * 6
        if kind == 0:
            fr = mac + [0x86, 0xdd] + [0x60, 0, 0, 0] + be16(len(tcp)) + [6, 64] + v6[0] + v6[1] + tcp
        elif kind == 1:
            ihl = 6 + int(rng.integers(0, 10))
            opts = [1] * (4 * (ihl - 5))
            fr = (mac + [0x08, 0x00] + [0x40 | ihl, 0] + be16(4 * ihl + len(udp)) + [0, 0, 0, 0, 64, 17, 0, 0] +
                  v4[0] + v4[1] + opts + udp)
        else:
            hop = [60, 0] + [0] * 6          # hop-by-hop, next: destination options
            dst = [17, 0] + [0] * 6          # destination options, next: UDP
            fr = (mac + [0x81, 0x00, 0x00, 0x05, 0x86, 0xdd] + [0x60, 0, 0, 0] +
                  be16(len(hop) + len(dst) + len(udp)) + [0, 64] + v6[0] + v6[1] + hop + dst + udp)
        assert len(fr) <= STRIDE
        out[i, :len(fr)] = fr
        lens[i] = len(fr)
    return out, lens


def reads_past_64(slot, ln):
    """The frame classes the 64-byte window cannot finish (CPU side)."""
    et = (int(slot[12]) << 8) | int(slot[13])
    if et in (0x8100, 0x88a8) and ln >= 18:
        return True
    if et == 0x0800 and ln >= 34 and (int(slot[14]) & 0xf) != 5:
        return True
    return et == 0x86dd and ln >= 74 and int(slot[20]) == 6


@pytest.mark.parametrize("mix", ["fuzz", "far"])
def test_descs_window_128(G, mixed, mix):
    rules, _, data, lens = mixed
    data, lens = data.copy(), lens.copy()
    if mix == "far":
        slots = data.reshape(-1, STRIDE)
        far, flens = far_frames(rules, len(lens) // 5 + 1, 5)
        slots[::5] = far
        lens[::5] = flens
        share = np.mean([reads_past_64(s, l) for s, l in zip(slots, lens)])
        assert share >= 0.1, share
    run_case(G, X.VARIANT_FEATURES["xdpfilt_dny_all"], rules, data, lens, STRIDE, 8192, 8192 - 777,
             want_path=G.Filter.PATH_PIPELINE, window=128)


def test_descs_window_64_deferred_walk(G, mixed):
    """The same far mix through the default 64-byte window: every such frame
    takes the deferred walk."""
    rules, _, data, lens = mixed
    data, lens = data.copy(), lens.copy()
    slots = data.reshape(-1, STRIDE)
    far, flens = far_frames(rules, len(lens) // 5 + 1, 6)
    slots[::5] = far
    lens[::5] = flens
    share = np.mean([reads_past_64(s, l) for s, l in zip(slots, lens)])
    assert share >= 0.1, share
    run_case(G, X.VARIANT_FEATURES["xdpfilt_dny_all"], rules, data, lens, STRIDE, 8192, 8192 - 777,
             want_path=G.Filter.PATH_PIPELINE)


# ---- 6: hit log and repeats
def slots_for(capacity, spb, lf):
    """nslots of a hash map (xfg_table.c: buckets_for)."""
    return (int(capacity / (spb * lf)) + 1) * spb


@pytest.mark.parametrize("hot", [False, True])
def test_descs_hit_log_and_repeats(G, hot):
    n = 1 << 17
    caps = dict(ipv4_capacity=8000, ipv6_capacity=2000, eth_capacity=1000)
    rules, pool = X.random_rules(91, n4=5000, n6=600, ne=24, nports=40)
    r = rules.prepared()
    # launch_batch turns the hit log on for a kind-1 launch when there are
    # more keys than XFG_LOG_MIN_KEYS, more counters than direct LDS
    # counters (XFG_DCNT_MAX) and gbase[3] + 65536 <= n
    nkeys = len(r.v4_keys) + len(r.v6_keys) + len(r.eth_keys)
    gbase3 = (slots_for(8000, layout_const("XFG_SLOTS_V4"), 0.6) + 1 +
              slots_for(2000, layout_const("XFG_SLOTS_V6"), 0.45) + 1 +
              slots_for(1000, layout_const("XFG_SLOTS_ETH"), 0.55) + 1)
    assert nkeys > layout_const("XFG_LOG_MIN_KEYS") and nkeys > layout_const("XFG_DCNT_MAX")
    assert gbase3 > layout_const("XFG_DCNT_MAX") and gbase3 + 65536 <= n
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    data, lens = X.gen_fuzz(17, n, STRIDE, rules, pool)
    if hot:   # every descriptor names one frame: one ruled destination
        slots = data.reshape(n, STRIDE)
        k = int(np.flatnonzero((lens >= 60) & (slots[:, 12] == 8) & (slots[:, 13] == 0) &
                               (slots[:, 14] == 0x45))[0])
        slots[k, 30:34] = r.v4_keys[np.flatnonzero(r.v4_vals & np.uint64(2))[0]]
        hot_data, hot_lens = slots[k].copy(), lens[k:k + 1].copy()
        umem = np.zeros(CHUNK * 4, np.uint8)
        umem[CHUNK + 16:CHUNK + 16 + STRIDE] = hot_data
        addr = np.full(n, CHUNK + 16, np.uint64)
        dlens = np.full(n, hot_lens[0], np.uint32)
        odata, olens, ostride = np.tile(hot_data, n), dlens, STRIDE
    else:
        umem, addr = umem_of(data, lens, STRIDE, seed=3, spare=0)
        dlens = lens
        odata, olens, ostride = data, lens, STRIDE
    assert umem.nbytes <= 32 << 20
    descs, first, mask = ring_of(addr, dlens, 1 << 18, (1 << 18) - 777)
    # a strided batch of another shape after them
    n2 = 3000
    data2, lens2 = X.gen_fuzz(18, n2, 128, rules, pool)
    ov, o1, st = X.run_oracle(feats, odata, olens, rules, stride=ostride)
    _, o2, st = X.run_oracle(feats, odata, olens, o1, stride=ostride, stats=st.copy())
    _, o3, st = X.run_oracle(feats, odata, olens, o2, stride=ostride, stats=st.copy())
    ov2, o4, st = X.run_oracle(feats, data2, lens2, o3, stride=128, stats=st.copy())
    f = G.Filter(feats, ndev=1, **caps)
    f.load_rules(rules)
    dev = Dev(f, umem, descs, n)
    for _ in range(3):                      # no counter read in between
        f.classify_descs(dev.umem.ptr, dev.descs.ptr, n, dev.v.ptr, first=first, mask=mask)
    assert f.last_path() == G.Filter.PATH_PIPELINE
    v2 = f.run(data2, lens2, stride=128)
    v = dev.v.download(np.zeros(n, np.uint8))
    np.testing.assert_array_equal(v, ov)
    np.testing.assert_array_equal(v2, ov2)
    check_all(G, f, rules, None, o4, st)
    f.close()


# ---- 7: the LDS Ethernet key table beside IPv4 and IPv6 rules
def test_descs_lds_ethernet_table(G):
    rules, pool = X.random_rules(55, n4=150, n6=60, ne=0, nports=30)
    c1 = X.c1_rules()
    rules.eth_keys, rules.eth_vals = c1.eth_keys, c1.eth_vals
    n = 4097
    data, lens = X.gen_fuzz(41, n, STRIDE, rules, pool)
    run_case(G, X.VARIANT_FEATURES["xdpfilt_dny_all"], rules, data, lens, STRIDE, 8192, 8192 - 777,
             want_path=G.Filter.PATH_PIPELINE)


# ---- 8: ABI
def test_descs_timed(G, mixed):
    rules, _, data, lens = mixed
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    n = len(lens)
    umem, addr = umem_of(data, lens, STRIDE, seed=9)
    descs, first, mask = ring_of(addr, lens, 8192, 8192 - 777)
    f = G.Filter(feats, ndev=1, descs_min_packets=1)
    f.load_rules(rules)
    dev = Dev(f, umem, descs, n)
    v = dev.classify(first, mask)
    tv = f.alloc(n)
    ms = f.classify_descs_timed(dev.umem.ptr, dev.descs.ptr, n, tv.ptr, 2, first=first, mask=mask)
    assert ms > 0
    assert f.last_path() == G.Filter.PATH_PIPELINE
    np.testing.assert_array_equal(tv.download(np.zeros(n, np.uint8)), v)
    ov, orules, ost = X.run_oracle(feats, data, lens, rules, stride=STRIDE)
    np.testing.assert_array_equal(v, ov)
    np.testing.assert_array_equal(f.stats(), ost * 3)
    with pytest.raises(OSError) as e:
        f.classify_descs_timed(dev.umem.ptr, dev.descs.ptr, n, tv.ptr, 0, first=first, mask=mask)
    assert e.value.errno == errno.EINVAL
    with pytest.raises(OSError) as e:
        f.classify_descs_timed(dev.umem.ptr, dev.descs.ptr, n, tv.ptr, 2, mask=1000)
    assert e.value.errno == errno.EINVAL
    f.close()


# ---- 9: the steady state of the pipeline: every wave takes several tiles
@pytest.mark.parametrize("window", [64, 128])
def test_descs_waves_take_several_tiles(G, mixed, window):
    """launch_batch caps the grid at the resident workgroups, so only a batch
    with more tiles than the device holds waves makes a wave loop: stage D's
    loads two tiles ahead, the records of one iteration consumed in the next,
    the prologue's second record and the drain.  2^20 + 65 descriptors (the
    last tile holds one packet) name the shared frames at random through a
    wrapping ring whose other entries are 0xFF bytes."""
    import torch
    rules, _, data, lens = mixed
    feats = X.VARIANT_FEATURES["xdpfilt_dny_all"]
    m, n = len(lens), (1 << 20) + 65
    # a CU holds at most 32 waves (8 a SIMD), so the grid has at most
    # 32 * CUs of them whatever the kernel's occupancy: with more than twice
    # as many tiles every wave takes two at least, most of them more
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (n + 63) // 64
    assert tiles > 2 * 32 * ncu, (tiles, ncu)
    fi = np.random.default_rng(window).integers(0, m, n)
    big_lens = lens[fi]
    ov, orules, ost = X.run_oracle(feats, data.reshape(m, STRIDE)[fi].reshape(-1), big_lens, rules,
                                   stride=STRIDE)
    umem, addr = umem_of(data, lens, STRIDE, seed=window)
    entries = 1 << 21
    descs, first, mask = ring_of(addr[fi], big_lens, entries, entries - 777, fill=0xFF)
    f = G.Filter(feats, ndev=1, window=window)
    f.load_rules(rules)
    v = Dev(f, umem, descs, n).classify(first, mask)
    assert f.last_path() == G.Filter.PATH_PIPELINE
    check_all(G, f, rules, ov, orules, ost, v)
    f.close()

"""Steered egress of multi-buffer packets (xfg_steer_frags_egress,
xfg_steer_frags.hip): every live record of a packet to the TX ring of its head
frame's queue, or to the fill ring.

Every comparison is exact against tests/steerfragmodel.py, whose head queues
are steermodel.py's (held equal to the reference's programs by
test_steer_reference.py); test_gpu_steer_frags_reference.py beside this file
takes its expected queues from the reference directly.  As in test_gpu_steer.py
a case's frames are a pool of distinct frames in a UMEM of random bytes and
records that name them -- so a continuation record's chunk holds another flow's
complete headers -- and every TX ring, the fill ring, queue_of, the counts and
the UMEM are prefilled with 0xA5 (the UMEM with its frames) and compared whole.
"""
import functools

import numpy as np
import pytest

import steerfragmodel as F
import steermodel as M
from test_gpu_egress import A5, Rings, pow2_at_least, slots
from test_gpu_steer import (MODES, PASS, T, classified, flows_64, hand_pool, random_pool,  # noqa: F401
                            umem_of_pool)

pytestmark = pytest.mark.gpu

NONE = F.VERDICT_NONE
OTHERS = np.array([0, 1, 3, 4], np.uint8)
SIZES = [T - 1, T, T + 1, 3 * T + 7]
QUEUES = [1, 2, 7, 64]
SHAPES = ["single", "three", "random"]


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


def plens_of(n, shape, seed=0):
    """Packet lengths that cover n records."""
    if shape == "single":
        return np.ones(n, np.int64)
    if shape == "three":
        return np.full(n // 3 + 1, 3, np.int64)
    return np.random.default_rng(1000 + n + seed).integers(1, 19, n)


def verdicts(n, seed=0, none=0.0):
    """A byte a record, drawn record by record (so a continuation's byte
    differs from its head's more often than not): 60 % PASS."""
    rng = np.random.default_rng(8 * n + seed)
    v = OTHERS[rng.integers(0, len(OTHERS), n)]
    v[rng.random(n) < 0.6] = PASS
    v[rng.random(n) < none] = NONE
    return v


def option_words(plens, n):
    """XDP_PKT_CONTD by the packet lengths, and on every fifth record a bit a
    TX record must not carry."""
    return F.opts_of_packet_lengths(plens, n) | np.where(np.arange(n) % 5 == 4, 1 << 16, 0).astype(np.uint32)


def launch(G, f, single, umem, addr, lens, opts, v, nq, mode, avail, skip_queue, kind, rot, fill, queue_of,
           flags):
    """One call; returns (counts, tx, fill, queue_of, umem) as downloaded, and
    the prefilled host copies and the rings."""
    n = len(v)
    rings = Rings(n, kind, rot)
    rx_e, tx_e, fill_e = rings.entries
    rx_h = np.full((max(rx_e, 1), 2), A5, np.uint64)
    rec = np.empty((n, 2), np.uint64)
    rec[:, 0] = addr
    rec[:, 1] = lens.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    rx_h[slots(rings.first[0], n, rings.mask[0])] = rec
    tx_h = np.full((nq, max(tx_e, 1), 2), A5, np.uint64)
    fill_h = np.full(max(fill_e, 1), A5, np.uint64)
    qof_h = np.full(n + 16, 0xA5, np.uint8)
    cnt_h = np.full(nq + 3, A5, np.uint64)
    tx_first = [(rings.first[1] + 3 * q) & 0xffffffff if kind == "ring" else 0 for q in range(nq)]
    bufs = [f.alloc(a.nbytes) for a in (umem, rx_h, tx_h, fill_h, qof_h, cnt_h)] + [f.alloc(max(n, 16))]
    d_u, d_rx, d_tx, d_fill, d_qof, d_c, d_v = bufs
    try:
        for d, a in zip(bufs, (umem, rx_h, tx_h, fill_h, qof_h, cnt_h)):
            d.upload(a)
        if n:
            d_v.upload(np.ascontiguousarray(v))
        queues = [(d_tx.ptr + q * tx_h[0].nbytes, tx_first[q], rings.mask[1]) for q in range(nq)]
        call = f.steer_egress if single else f.steer_frags_egress
        call(d_u.ptr, d_rx.ptr, n, d_v.ptr, d_c.ptr, queues, avail=avail, mode=mode, skip_queue=skip_queue,
             fill_ptr=d_fill.ptr if fill else None, rx_first=rings.first[0], rx_mask=rings.mask[0],
             fill_first=rings.first[2], fill_mask=rings.mask[2], queue_of_ptr=d_qof.ptr if queue_of else None,
             flags=flags)
        f.sync()
        got = (d_c.download(np.zeros_like(cnt_h)), d_tx.download(np.zeros_like(tx_h)),
               d_fill.download(np.zeros_like(fill_h)), d_qof.download(np.zeros_like(qof_h)),
               d_u.download(np.zeros_like(umem)))
    finally:
        for b in bufs:
            b.free()
    return got, (cnt_h, tx_h, fill_h, qof_h), rings, tx_first


def check(G, f, umem, addr, start, lens, opts, v, nq, want, mode=M.L4_HASH, avail=None, skip_queue=0,
          kind="array", rot=0, fill=True, queue_of=True, flags=0, also_single=False):
    """One call over the records; counts, every ring, queue_of and the UMEM
    whole against @want = (tx, fill, counts, queue_of)."""
    n = len(v)
    want_tx, want_fill, want_counts, want_qof = want
    got, (cnt_h, tx_h, fill_h, qof_h), rings, tx_first = launch(
        G, f, False, umem, addr, lens, opts, v, nq, mode, avail, skip_queue, kind, rot, fill, queue_of, flags)
    got_c, got_tx, got_fill, got_qof, got_umem = got
    cnt_h[:nq + 2] = want_counts
    np.testing.assert_array_equal(got_c, cnt_h)
    assert int(want_counts[:nq + 1].sum()) == int((np.asarray(v) != NONE).sum())
    if queue_of:
        qof_h[:n] = want_qof
    np.testing.assert_array_equal(got_qof, qof_h)
    for q in range(nq):
        tx_h[q][slots(tx_first[q], len(want_tx[q]), rings.mask[1])] = want_tx[q]
    np.testing.assert_array_equal(got_tx, tx_h)
    if fill:
        fill_h[slots(rings.first[2], len(want_fill), rings.mask[2])] = want_fill
    np.testing.assert_array_equal(got_fill, fill_h)
    want_umem = umem
    if flags & G.EGRESS_SWAP_MACS:
        _, head, _ = F.packets(v, opts)
        want_umem = umem.copy()
        at = np.asarray(start)[head & (np.asarray(v) == PASS)][:, None] + np.arange(12)
        want_umem[at] = umem[at][:, [6, 7, 8, 9, 10, 11, 0, 1, 2, 3, 4, 5]]
    np.testing.assert_array_equal(got_umem, want_umem)
    if also_single:
        one, _, _, _ = launch(G, f, True, umem, addr, lens, opts, v, nq, mode, avail, skip_queue, kind, rot,
                              fill, queue_of, flags & ~G.EGRESS_MULTIBUF)
        for a, b in zip(got, one):
            np.testing.assert_array_equal(a, b)
    return want_counts


def run(G, f, pool, fid, opts, v, nq, mode=M.L4_HASH, avail=None, skip_queue=0, seed=3, precheck=None, **kw):
    umem, paddr, pstart, plens = umem_of_pool(pool, seed)
    addr, lens = paddr[fid], plens[fid]
    want = F.steer_frags_model(pool, addr, lens, opts, v, nq, mode, avail, skip_queue, fid=fid)
    if precheck:
        precheck(want, opts, v)
    return check(G, f, umem, addr, pstart[fid], lens, opts, v, nq, want, mode=mode, avail=avail,
                 skip_queue=skip_queue, **kw)


def fids(n, npool, seed=0):
    return np.random.default_rng(100 + n + seed).integers(0, npool, n)


# ---- 1: sizes x queue counts x packet shapes (mode and ring form by turns)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("nq", QUEUES)
@pytest.mark.parametrize("n", SIZES)
def test_partition(G, filt, n, nq, shape):
    k = SIZES.index(n) + QUEUES.index(nq) + SHAPES.index(shape)
    pool = random_pool()
    single = shape == "single"
    v = verdicts(n, k, none=0.0 if single else 0.03)
    run(G, filt, pool, fids(n, len(pool)), option_words(plens_of(n, shape), n), v, nq, mode=MODES[k % 3],
        skip_queue=nq - 1, kind=["array", "ring"][(k // 3) % 2], rot=k, also_single=single,
        flags=[0, G.EGRESS_MULTIBUF][k % 2])


# ---- 2: all three modes, both ring forms
@pytest.mark.parametrize("kind", ["array", "ring"])
@pytest.mark.parametrize("mode", MODES)
def test_modes(G, filt, mode, kind):
    n = 3 * T + 7
    pool = random_pool()
    run(G, filt, pool, fids(n, len(pool), 1), option_words(plens_of(n, "random", 1), n), verdicts(n, 1, 0.02),
        7, mode=mode, kind=kind, rot=mode, skip_queue=3)


def test_hand_written_rows_as_heads(G, filt):
    """The CPU tests' rows, one a branch of the programs, as heads of
    three-record packets: refused heads count per packet."""
    pool = hand_pool() + random_pool()[:64]
    n = T + 77
    fid = np.random.default_rng(77).integers(0, len(pool), n)
    fid[0:3 * len(hand_pool()):3] = np.arange(len(hand_pool()))
    v = verdicts(n, 2)
    v[0:3 * len(hand_pool()):3] = PASS
    want = run(G, filt, pool, fid, option_words(plens_of(n, "three"), n), v, 7, skip_queue=6, kind="ring", rot=2)
    assert 4 <= want[8] < want[6]


# ---- 3: placements
N3 = 3 * T + 7
PLACEMENTS = {
    # a packet ending on a tile's last record, a head that is a tile's first
    "tile_edges": ([T - 4, 4, 3], N3, 0),
    # heads in a wave's last lane, their continuations in the next wave (or pass)
    "wave_last_lane": ([63] + [64] * 40, N3, 0),
    # 70 records straddling a tile boundary, the head 67 before it: two steps back
    "straddle_70": ([T - 67, 70], N3, 0),
    # T + 5 records from record 3 on
    "tile_and_5": ([3, T + 5], 2 * T + 50, 0),
    # 2T + 3 records: tile 1 holds no head
    "two_tiles_and_3": ([5, 2 * T + 3], N3 + 93, 0),
    # the walk back crosses the RX ring's wrap (rot 1: the RX ring wraps mid-batch)
    "wrap": ([1500, 600], N3, 1),
}


@pytest.mark.parametrize("name", list(PLACEMENTS))
@pytest.mark.parametrize("head", ["pass", "other"])
def test_placements(G, filt, name, head):
    first, n, rot = PLACEMENTS[name]
    plens = np.concatenate([first, plens_of(n, "three")])
    opts = option_words(plens, n)
    v = verdicts(n, 3)
    long_head = int(np.sum(first[:-1]))
    v[long_head] = PASS if head == "pass" else 1
    kind = "ring" if name == "wrap" else "array"
    if name == "wrap":
        r = Rings(n, kind, rot)
        wrap_at = (r.mask[0] + 1) - (r.first[0] & r.mask[0])     # the first record in slot 0
        assert long_head < wrap_at < T < long_head + first[-1]

    def pre(want, opts, v):
        _, hd, head_of = F.packets(v, opts)
        assert int((head_of == long_head).sum()) == first[-1]
        if name == "two_tiles_and_3":
            assert not hd[T:2 * T].any()

    run(G, filt, random_pool(), fids(n, len(random_pool()), 3), opts, v, 7, kind=kind, rot=rot, precheck=pre,
        skip_queue=2)


# ---- 4: liveness
@pytest.mark.parametrize("where", ["middle", "tile_last", "tile_first", "all"])
def test_verdict_none_runs(G, filt, where):
    n = N3
    opts = option_words(plens_of(n, "random", 4), n)
    v = verdicts(n, 4)
    runs = {"middle": [(700, 790), (T + 100, T + 101)], "tile_last": [(T - 1, T), (2 * T - 9, 2 * T)],
            "tile_first": [(T, T + 1), (2 * T, 2 * T + 70)], "all": [(0, n)]}[where]
    for a, b in runs:
        v[a:b] = NONE

    def pre(want, opts, v):
        live, head, _ = F.packets(v, opts)
        if where != "all":
            # a packet cut by a run: the record behind the run is a head though its predecessor goes on
            assert any(b < n and live[b] and head[b] and (opts[b - 1] & F.CONTD) for _, b in runs)

    run(G, filt, random_pool(), fids(n, len(random_pool()), 4), opts, v, 7, kind="ring", rot=2, precheck=pre)


# ---- 5: continuation records
def test_continuations_hold_other_flows_and_other_verdicts(G, filt):
    n = N3
    pool = random_pool()
    fid = fids(n, len(pool), 5)
    opts = option_words(plens_of(n, "random", 5), n)
    v = verdicts(n, 5)

    def pre(want, opts, v):
        live, head, head_of = F.packets(v, opts)
        cont = np.flatnonzero(live & ~head)
        assert len(cont) > n // 2
        assert np.mean(v[cont] != v[head_of[cont]]) > 0.3
        # steered by their own bytes most of them would take another queue
        own = F.steer_frags_model(pool, np.zeros(n, np.uint64), np.ones(n), np.zeros(n, np.uint32),
                                  np.full(n, PASS, np.uint8), 64, fid=fid)[3]
        assert np.mean(own[cont] != own[head_of[cont]]) > 0.9

    run(G, filt, pool, fid, opts, v, 64, precheck=pre)


# ---- 6: pointers and flags
@pytest.mark.parametrize("mode", MODES)
def test_swap_macs(G, filt, mode):
    """Distinct frames: only the heads of PASS packets are swapped."""
    pool = random_pool()[:T + 40] + hand_pool()
    n = len(pool)
    fid = np.random.default_rng(12).permutation(n)
    run(G, filt, pool, fid, option_words(plens_of(n, "random", 6), n), verdicts(n, 6, 0.02), 7, mode=mode,
        skip_queue=3, flags=G.EGRESS_SWAP_MACS | G.EGRESS_MULTIBUF, kind="ring")


def test_no_fill_ring(G, filt):
    n = N3
    run(G, filt, random_pool(), fids(n, len(random_pool()), 7), option_words(plens_of(n, "three"), n),
        verdicts(n, 7, 0.02), 7, fill=False, kind="ring")


def test_no_queue_of(G, filt):
    n = N3
    run(G, filt, random_pool(), fids(n, len(random_pool()), 8), option_words(plens_of(n, "random", 8), n),
        verdicts(n, 8), 3, queue_of=False, mode=M.L4_SPORT)


def test_empty_batch_zeroes_the_counts(G, filt):
    run(G, filt, random_pool()[:8], np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint8), 5)


# ---- 7: 64 single-record heads to 64 queues, then long packets
def test_64_queues_a_wave_then_long_packets(G, filt):
    pool = flows_64() + random_pool()[:512]
    n = N3
    rng = np.random.default_rng(6464)
    plens = np.concatenate([np.ones(64, np.int64), [100, 300, 64, 65, 1000], plens_of(n, "random", 9)])
    fid = 64 + rng.integers(0, 512, n)
    fid[:64] = rng.permutation(64)
    v = verdicts(n, 9)
    v[:64 + 5] = PASS
    heads = np.concatenate([[0], np.cumsum(plens)[:-1]])
    v[heads[64:69]] = PASS

    def pre(want, opts, v):
        assert sorted(want[3][:64].tolist()) == list(range(64))

    run(G, filt, pool, fid, option_words(plens, n), v, 64, precheck=pre)


# ---- 8: the random-flow case: every one of 64 queues, none above half
SPREAD_SEED = 9


def test_random_flows_reach_every_queue(G, filt):
    n = N3
    pool = random_pool()
    fid = np.random.default_rng(SPREAD_SEED).permutation(len(pool))
    fid = np.concatenate([fid, fid[:n - len(fid)]])
    v = np.full(n, PASS, np.uint8)

    def spread(want, opts, v):
        per = want[2][:64].astype(np.int64)
        assert per.min() >= 1 and per.max() <= n // 2

    run(G, filt, pool, fid, option_words(plens_of(n, "random", 10), n), v, 64, precheck=spread, kind="ring")


# ---- 9: more tiles than workgroups
def test_more_tiles_than_the_grid(G, filt):
    import torch
    n = 2**22 + 13
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert (n + T - 1) // T > 4 * ncu
    pool = random_pool()
    run(G, filt, pool, fids(n, len(pool), 5), option_words(plens_of(n, "three"), n), verdicts(n, 11, 0.01), 3,
        skip_queue=1)


# ---- 10: composition
def frag_case(classified_case, plens):
    """The classified fixture's records cut into packets: the verdict bytes
    xfg_classify_descs_frags leaves (the head's on every record of a complete
    packet, VERDICT_NONE behind the last end of packet)."""
    _, umem, addr, lens, frames, ov = classified_case
    n = len(lens)
    opts = F.opts_of_packet_lengths(plens, n)
    _, _, head_of = F.packets(np.zeros(n, np.uint8), opts)
    v = ov[head_of].astype(np.uint8)
    done = int(np.flatnonzero((opts & F.CONTD) == 0)[-1]) + 1
    v[done:] = NONE
    return opts, v, done


@pytest.mark.parametrize("where", ["library_stream", "caller_stream"])
def test_classify_frags_then_steer_without_sync(G, classified, where):  # noqa: F811
    import torch
    f, umem, addr, lens, frames, ov = classified
    n = len(lens)
    plens = np.concatenate([np.random.default_rng(5).integers(1, 6, n // 4), [n]])
    opts, v, done = frag_case(classified, plens)
    assert done < n and 0 < np.count_nonzero(v[:done] == PASS) < done
    stream = torch.cuda.Stream() if where == "caller_stream" else None
    sp = stream.cuda_stream if stream else None
    nq, E = 8, max(8192, pow2_at_least(n))
    want_tx, want_fill, want_counts, want_qof = F.steer_frags_model(frames[:done], addr[:done], lens[:done],
                                                                    opts[:done], v[:done], nq)
    tx_h = np.full((nq, E, 2), A5, np.uint64)
    fill_h = np.full(E, A5, np.uint64)
    cnt_h = np.full(nq + 3, A5, np.uint64)
    qof_h = np.full(n + 16, 0xA5, np.uint8)
    descs = np.empty((n, 2), np.uint64)
    descs[:, 0], descs[:, 1] = addr, lens.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    hosts = (umem, descs, tx_h, fill_h, cnt_h, qof_h)
    bufs = [f.alloc(a.nbytes) for a in hosts] + [f.alloc(n)]
    d_u, d_rx, d_tx, d_fill, d_c, d_qof, d_v = bufs
    try:
        for d, a in zip(bufs, hosts):
            d.upload(a)
        d_v.upload(np.full(n, 7, np.uint8))
        f.sync()
        counts = f.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, stream=sp)
        assert counts[1] == done
        queues = [(d_tx.ptr + q * tx_h[0].nbytes, E - 100 + q, E - 1) for q in range(nq)]
        f.steer_frags_egress(d_u.ptr, d_rx.ptr, counts[1], d_v.ptr, d_c.ptr, queues, fill_ptr=d_fill.ptr,
                             fill_first=0xfffffff0, fill_mask=E - 1, queue_of_ptr=d_qof.ptr, stream=sp,
                             flags=G.EGRESS_MULTIBUF)
        if sp:
            torch.cuda.synchronize()
        f.sync()
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8))[:done], v[:done])
        cnt_h[:nq + 2] = want_counts
        np.testing.assert_array_equal(d_c.download(np.zeros_like(cnt_h)), cnt_h)
        qof_h[:done] = want_qof
        np.testing.assert_array_equal(d_qof.download(np.zeros_like(qof_h)), qof_h)
        for q in range(nq):
            tx_h[q][slots(E - 100 + q, len(want_tx[q]), E - 1)] = want_tx[q]
        fill_h[slots(0xfffffff0, len(want_fill), E - 1)] = want_fill
        np.testing.assert_array_equal(d_tx.download(np.zeros_like(tx_h)), tx_h)
        np.testing.assert_array_equal(d_fill.download(np.zeros_like(fill_h)), fill_h)
    finally:
        for b in bufs:
            b.free()


def test_steer_over_the_flat_array_of_classify_socks_frags(G, classified):  # noqa: F811
    """A poll round of a few SG sockets with trailing incomplete packets:
    sk->flat as a plain array, its VERDICT_NONE bytes keeping the sockets
    apart."""
    f, umem, addr, lens, frames, ov = classified
    n = len(lens)
    per = [0, 64, 1, 2047, 0, 900, 1000, 85, 0]
    assert sum(per) == n
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    rng = np.random.default_rng(9)
    opts = np.full(n, F.CONTD, np.uint32)
    v = np.full(n, NONE, np.uint8)
    for s, c in enumerate(per):
        if c > 3:
            o = F.opts_of_packet_lengths(np.concatenate([rng.integers(1, 6, c // 4), [c]]), c)
            opts[off[s]:off[s + 1]] = o
            done = int(np.flatnonzero((o & F.CONTD) == 0)[-1]) + 1
            assert done < c                                   # a trailing incomplete packet
            _, _, head_of = F.packets(np.zeros(done, np.uint8), o[:done])
            v[off[s]:off[s] + done] = ov[off[s] + head_of]
    nq, E = 3, max(8192, pow2_at_least(n))
    want_tx, want_fill, want_counts, want_qof = F.steer_frags_model(frames, addr, lens, opts, v, nq, M.L4_DPORT)
    assert want_counts[:nq].min() > 0 and 0 < int((v == NONE).sum()) < n
    tx_h = np.full((nq, E, 2), A5, np.uint64)
    fill_h = np.full(E, A5, np.uint64)
    cnt_h = np.full(nq + 3, A5, np.uint64)
    qof_h = np.full(n + 16, 0xA5, np.uint8)
    descs = np.empty((n, 2), np.uint64)
    descs[:, 0], descs[:, 1] = addr, lens.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    flat_h = np.full((n, 2), A5, np.uint64)
    hosts = (umem, descs, tx_h, fill_h, cnt_h, qof_h, flat_h)
    bufs = [f.alloc(a.nbytes) for a in hosts] + [f.alloc(n)]
    d_u, d_rx, d_tx, d_fill, d_c, d_qof, d_flat, d_v = bufs
    try:
        for d, a in zip(bufs, hosts):
            d.upload(a)
        d_v.upload(np.full(n, 7, np.uint8))
        f.sync()
        socks = [dict(rx_descs=d_rx.ptr + 16 * int(off[s]) if c else None, count=c, tx_descs=None,
                      fill_addrs=None) for s, c in enumerate(per)]
        f.classify_socks_frags(d_u.ptr, socks, d_v.ptr, flat_ptr=d_flat.ptr)
        queues = [(d_tx.ptr + q * tx_h[0].nbytes, E - 100 + q, E - 1) for q in range(nq)]
        f.steer_frags_egress(d_u.ptr, d_flat.ptr, n, d_v.ptr, d_c.ptr, queues, mode=M.L4_DPORT,
                             fill_ptr=d_fill.ptr, fill_first=0xfffffff0, fill_mask=E - 1,
                             queue_of_ptr=d_qof.ptr)
        f.sync()
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8)), v)
        cnt_h[:nq + 2] = want_counts
        np.testing.assert_array_equal(d_c.download(np.zeros_like(cnt_h)), cnt_h)
        qof_h[:n] = want_qof
        np.testing.assert_array_equal(d_qof.download(np.zeros_like(qof_h)), qof_h)
        for q in range(nq):
            tx_h[q][slots(E - 100 + q, len(want_tx[q]), E - 1)] = want_tx[q]
        fill_h[slots(0xfffffff0, len(want_fill), E - 1)] = want_fill
        np.testing.assert_array_equal(d_tx.download(np.zeros_like(tx_h)), tx_h)
        np.testing.assert_array_equal(d_fill.download(np.zeros_like(fill_h)), fill_h)
    finally:
        for b in bufs:
            b.free()

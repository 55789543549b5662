"""Forwarded egress of multi-buffer packets (xfg_forward_frags_egress,
xfg_forward_frags.hip): every live record of a packet to the TX ring the
program gives its head buffer -- a port's, the head rewritten, or the stack
ring -- or to the fill ring.

Every comparison is exact against tests/fwdfragmodel.py (steerfragmodel's
packet rules over fwdmodel's program, both held equal to the reference on their
own); test_gpu_forward_frags_reference.py beside this file takes its expected
values from the reference directly.  Every record has a chunk of its own in a
UMEM of random bytes, and a continuation's chunk holds a whole frame of another
flow.  Every ring, queue_of, reason_of and the counts are uploaded as 0xA5
bytes and compared whole against a copy with the expected entries written in,
and the whole UMEM is compared, so a stray write or a second decrement shows.
The cases' inputs are fwdfragmodel's; tests/test_forward_frags_model.py asserts,
without a GPU, the condition each is named for.
"""
import numpy as np
import pytest

import fwdcorpus as K
import fwdfragmodel as W
import fwdmodel as M
from test_gpu_egress import A5, Rings, pow2_at_least, slots
from test_gpu_steer import classified  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

T, N3, PASS, NONE = W.T, W.N3, W.PASS, W.NONE


@pytest.fixture(scope="module")
def G():
    import xfgpu
    return xfgpu


@pytest.fixture(scope="module")
def filt(G):
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=1)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fibs(G, filt):
    """One FIB a port count, built on first use and alive together."""
    made = {}

    def get(nports):
        if nports not in made:
            routes, nexthops = K.fib_of(nports)
            made[nports] = G.Fib(filt, routes, nexthops)
        return made[nports]

    yield get
    for fib in made.values():
        fib.free()


def launch(G, f, fib, single, umem, addr, lens, opts, v, ifx, kind, rot, fill, queue_of, reason_of, flags,
           calls=1):
    """@calls calls over the same buffers; returns what they leave, the
    prefilled host copies and the rings."""
    n, P = len(v), len(ifx)
    rings = Rings(n, kind, rot)
    rx_e, tx_e, fill_e = rings.entries
    rx_h = np.full((max(rx_e, 1), 2), A5, np.uint64)
    rec = np.empty((n, 2), np.uint64)
    rec[:, 0] = addr
    rec[:, 1] = lens.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    rx_h[slots(rings.first[0], n, rings.mask[0])] = rec
    tx_h = np.full((P + 1, max(tx_e, 1), 2), A5, np.uint64)
    fill_h = np.full(max(fill_e, 1), A5, np.uint64)
    qof_h = np.full(n + 16, 0xA5, np.uint8)
    rof_h = np.full(n + 16, 0xA5, np.uint8)
    cnt_h = np.full(P + 2 + M.REASONS + 1, A5, np.uint64)
    tx_first = [(rings.first[1] + 3 * q) & 0xffffffff if kind == "ring" else 0 for q in range(P + 1)]
    hosts = (umem, rx_h, tx_h, fill_h, qof_h, rof_h, cnt_h)
    bufs = [f.alloc(a.nbytes) for a in hosts] + [f.alloc(max(n, 16))]
    d_u, d_rx, d_tx, d_fill, d_qof, d_rof, d_c, d_v = bufs
    try:
        for d, a in zip(bufs, hosts):
            d.upload(a)
        if n:
            d_v.upload(np.ascontiguousarray(v))
        q_at = [(d_tx.ptr + q * tx_h[0].nbytes, tx_first[q], rings.mask[1]) for q in range(P + 1)]
        ports = [(ifx[q],) + q_at[q] for q in range(P)]
        call = f.forward_egress if single else f.forward_frags_egress
        for _ in range(calls):
            call(d_u.ptr, d_rx.ptr, n, d_v.ptr, d_c.ptr, fib, ports, q_at[P],
                 fill_ptr=d_fill.ptr if fill else None, rx_first=rings.first[0], rx_mask=rings.mask[0],
                 fill_first=rings.first[2], fill_mask=rings.mask[2],
                 queue_of_ptr=d_qof.ptr if queue_of else None, reason_of_ptr=d_rof.ptr if reason_of else None,
                 flags=flags)
        f.sync()
        got = [d.download(np.zeros_like(a)) for d, a in zip(bufs, hosts)]
    finally:
        for b in bufs:
            b.free()
    return got, (tx_h, fill_h, qof_h, rof_h, cnt_h), rings, tx_first


def compare(got, blank, rings, tx_first, want, n, P, fill=True, queue_of=True, reason_of=True, under=None):
    """What a call left against @want = (tx, fill, counts, queue_of, reason_of,
    umem), written into the 0xA5 copies (over @under's ring entries: those of
    a call before it)."""
    got_umem, _, got_tx, got_fill, got_qof, got_rof, got_c = got
    tx_h, fill_h, qof_h, rof_h, cnt_h = blank
    if under:
        for q in range(P + 1):
            tx_h[q][slots(tx_first[q], len(under[0][q]), rings.mask[1])] = under[0][q]
        fill_h[slots(rings.first[2], len(under[1]), rings.mask[2])] = under[1]
    want_tx, want_fill, want_counts, want_qof, want_rof, want_umem = want
    cnt_h[:P + 2 + M.REASONS] = want_counts
    np.testing.assert_array_equal(got_c, cnt_h)
    if queue_of:
        qof_h[:n] = want_qof
    np.testing.assert_array_equal(got_qof, qof_h)
    if reason_of:
        rof_h[:n] = want_rof
    np.testing.assert_array_equal(got_rof, rof_h)
    for q in range(P + 1):
        tx_h[q][slots(tx_first[q], len(want_tx[q]), rings.mask[1])] = want_tx[q]
    np.testing.assert_array_equal(got_tx, tx_h)
    if fill:
        fill_h[slots(rings.first[2], len(want_fill), rings.mask[2])] = want_fill
    np.testing.assert_array_equal(got_fill, fill_h)
    np.testing.assert_array_equal(got_umem, want_umem)


def run(G, f, fibs, nports, fid, opts, v, kind="array", rot=0, fill=True, queue_of=True, reason_of=True,
        flags=0, also_single=False, seed=3):
    """One call over the records; everything against the model.  Returns the
    model's answer."""
    n = len(v)
    routes, nexthops = K.fib_of(nports)
    ifx = K.ifindexes(nports)
    umem, addr, lens, chunk, room = W.umem_of_records(nports, fid, seed)
    m = W.forward_frags_model(W.pool_of(nports), fid, addr, lens, opts, v, routes, nexthops, ifx)
    want = m[:5] + (W.umem_after(umem, fid, chunk, room, m[5], m[6]),)
    assert int(m[2][:nports + 2].sum()) == int((np.asarray(v) != NONE).sum())
    got, blank, rings, tx_first = launch(G, f, fibs(nports), False, umem, addr, lens, opts, v, ifx, kind, rot,
                                         fill, queue_of, reason_of, flags)
    compare(got, blank, rings, tx_first, want, n, nports, fill, queue_of, reason_of)
    if also_single:
        one, _, _, _ = launch(G, f, fibs(nports), True, umem, addr, lens, opts, v, ifx, kind, rot, fill, queue_of,
                              reason_of, 0)
        for a, b in zip(got, one):
            np.testing.assert_array_equal(a, b)
    return m


# ---- 1: sizes x port counts x packet shapes (ring form and flag by turns)
@pytest.mark.parametrize("shape", W.SHAPES)
@pytest.mark.parametrize("nports", W.PORTS)
@pytest.mark.parametrize("n", W.SIZES)
def test_partition(G, filt, fibs, n, nports, shape):
    k = W.SIZES.index(n) + W.PORTS.index(nports) + W.SHAPES.index(shape)
    single = shape == "single"
    v = W.verdicts(n, k, none=0.0 if single else 0.03)
    run(G, filt, fibs, nports, W.fids(n), W.option_words(W.plens_of(n, shape), n), v,
        kind=["array", "ring"][(k // 3) % 2], rot=k, also_single=single, flags=[0, G.EGRESS_MULTIBUF][k % 2])


# ---- 2: the carry in every position
@pytest.mark.parametrize("name", list(W.PLACEMENTS))
@pytest.mark.parametrize("head", ["pass", "other"])
def test_placements(G, filt, fibs, name, head):
    fid, opts, v, _ = W.placement(name, head)
    wrap = name == "wrap"
    run(G, filt, fibs, 8, fid, opts, v, kind="ring" if wrap else "array", rot=1 if wrap else 0)


# ---- 3: the hazard: a straddling packet's head is rewritten while later tiles place its tail
@pytest.mark.parametrize("ttl", [2, 1])
def test_every_boundary_straddled(G, filt, fibs, ttl):
    """TTL 2: every record on the head's port, the head left with TTL 1.  TTL
    1: every record on the stack ring with XFG_FWD_TTL, nothing written.  Once:
    what keeps a tile from reading a rewritten head is the design, not a loop."""
    fid, opts, v, heads = W.hazard(ttl)
    m = run(G, filt, fibs, 8, fid, opts, v, kind="ring", rot=ttl)
    for d in range(5):
        assert (m[4][heads + d] == (M.OK if ttl == 2 else M.TTL)).all()


def test_two_tiles_and_3_with_a_ttl_2_head(G, filt, fibs):
    fid, opts, v, h = W.placement("two_tiles_and_3", "pass", ttl=2)
    m = run(G, filt, fibs, 8, fid, opts, v)
    assert (m[4][h:h + 2 * T + 3] == M.OK).all() and len(set(m[3][h:h + 2 * T + 3].tolist())) == 1


# ---- 4: liveness
@pytest.mark.parametrize("where", list(W.NONE_RUNS))
def test_verdict_none_runs(G, filt, fibs, where):
    fid, opts, v = W.none_runs(where)
    run(G, filt, fibs, 8, fid, opts, v, kind="ring", rot=2)


# ---- 5: continuation records
def test_continuations_hold_other_ports_frames_and_other_verdicts(G, filt, fibs):
    """(test_forward_frags_model.py: forwarded by their own bytes most of them
    would take another queue, with TTL to spare, under another verdict byte.)"""
    n = N3
    run(G, filt, fibs, 63, W.fids(n, 5), W.option_words(W.plens_of(n, "random", 5), n), W.verdicts(n, 5))


def test_every_reason_on_a_packet_of_several_records(G, filt, fibs):
    fid, opts, v = W.every_reason()
    m = run(G, filt, fibs, 8, fid, opts, v, kind="ring")
    assert (m[2][10:] > 0).all()


# ---- 6: optional outputs
def test_no_fill_ring(G, filt, fibs):
    n = N3
    run(G, filt, fibs, 8, W.fids(n, 7), W.option_words(W.plens_of(n, "three"), n), W.verdicts(n, 7, 0.02),
        fill=False, kind="ring")


@pytest.mark.parametrize("given", [(False, True), (True, False), (False, False)])
def test_queue_of_and_reason_of_null(G, filt, fibs, given):
    n = N3
    run(G, filt, fibs, 8, W.fids(n, 8), W.option_words(W.plens_of(n, "random", 8), n), W.verdicts(n, 8),
        queue_of=given[0], reason_of=given[1])


def test_empty_batch_zeroes_the_counts(G, filt, fibs):
    run(G, filt, fibs, 8, np.zeros(0, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint8))


# ---- 7: a second call on the same UMEM: the model applied twice
def test_second_call_decrements_again(G, filt, fibs):
    n, nports = T + 77, 8
    routes, nexthops = K.fib_of(nports)
    ifx = K.ifindexes(nports)
    fid, opts, v = W.fids(n, 9), W.option_words(W.plens_of(n, "random", 9), n), W.verdicts(n, 9, 0.02)
    fid[:W.NSPECIAL] = W.TTL2 + np.arange(W.NSPECIAL)     # forwarded once, to the stack ring the second time
    umem, addr, lens, chunk, room = W.umem_of_records(nports, fid)
    pool = W.pool_of(nports)
    m1 = W.forward_frags_model(pool, fid, addr, lens, opts, v, routes, nexthops, ifx)
    # the second call's frames: a rewritten head's is its frame after the first
    pool2 = list(pool) + [m1[6][int(k)][2] if int(k) in m1[6] else pool[k] for k in range(len(pool))]
    fid2 = np.where(m1[5], fid + len(pool), fid)
    m2 = W.forward_frags_model(pool2, fid2, addr, lens, opts, v, routes, nexthops, ifx)
    assert 0 < m2[5].sum() < m1[5].sum() and m2[2][10 + M.TTL] > m1[2][10 + M.TTL]
    after1 = W.umem_after(umem, fid, chunk, room, m1[5], m1[6])
    after2 = W.umem_after(after1, fid2, chunk, room, m2[5], m2[6])
    got, blank, rings, tx_first = launch(G, filt, fibs(nports), False, umem, addr, lens, opts, v, ifx, "ring", 1,
                                         True, True, True, 0, calls=2)
    compare(got, blank, rings, tx_first, m2[:5] + (after2,), n, nports, under=m1)


# ---- 8: more tiles than workgroups: the tile loop's later tickets
def test_more_tiles_than_the_grid(G, filt, fibs):
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = (4 * ncu + 2) * T
    run(G, filt, fibs, 8, np.random.default_rng(5).integers(0, K.POOL, n), W.option_words(W.plens_of(n, "three"), n),
        W.verdicts(n, 11, 0.01))


# ---- 9: composition
def composed(G, classified_case, opts, v, n_call, classify):
    """The classified fixture's frames (a chunk a record) through @classify and
    then the forward call, nothing between them, over a FIB with a default
    route; the verdict bytes must come out as @v."""
    f, umem, addr, lens, frames, ov = classified_case
    n = len(lens)
    nports = 8
    routes, nexthops = K.fib_of(nports)
    routes = routes + ((0, 0, 1),)
    ifx = K.ifindexes(nports)
    E = max(8192, pow2_at_least(n))
    pool = [bytes(fr) for fr in frames]
    m = W.forward_frags_model(pool, np.arange(n_call), addr[:n_call], lens[:n_call], opts[:n_call], v[:n_call],
                              routes, nexthops, ifx)
    assert m[5].sum() > 0 and (m[2][:nports + 1] > 0).sum() >= 2
    want_umem = umem.copy()
    for i in np.flatnonzero(m[5]):
        at = int(addr[i] & np.uint64(W.ADDR48)) + int(addr[i] >> np.uint64(48))
        want_umem[at:at + len(pool[i])] = np.frombuffer(m[6][int(i)][2], np.uint8)
    tx_h = np.full((nports + 1, E, 2), A5, np.uint64)
    fill_h = np.full(E, A5, np.uint64)
    cnt_h = np.full(nports + 2 + M.REASONS + 1, A5, np.uint64)
    qof_h = np.full(n + 16, 0xA5, np.uint8)
    rof_h = np.full(n + 16, 0xA5, np.uint8)
    descs = np.empty((n, 2), np.uint64)
    descs[:, 0], descs[:, 1] = addr, lens.astype(np.uint64) | (opts.astype(np.uint64) << np.uint64(32))
    flat_h = np.full((n, 2), A5, np.uint64)
    hosts = (umem, descs, tx_h, fill_h, cnt_h, qof_h, rof_h, flat_h)
    bufs = [f.alloc(a.nbytes) for a in hosts] + [f.alloc(n)]
    d_u, d_rx, d_tx, d_fill, d_c, d_qof, d_rof, d_flat, d_v = bufs
    fib = G.Fib(f, routes, nexthops)
    try:
        for d, a in zip(bufs, hosts):
            d.upload(a)
        d_v.upload(np.full(n, 7, np.uint8))
        f.sync()
        q_at = [(d_tx.ptr + q * tx_h[0].nbytes, E - 100 + q, E - 1) for q in range(nports + 1)]
        ports = [(ifx[q],) + q_at[q] for q in range(nports)]
        rx_ptr, count, sp, wait = classify(f, d_u, d_rx, d_flat, d_v)
        assert count == n_call
        f.forward_frags_egress(d_u.ptr, rx_ptr, count, d_v.ptr, d_c.ptr, fib, ports, q_at[nports],
                               fill_ptr=d_fill.ptr, fill_first=0xfffffff0, fill_mask=E - 1,
                               queue_of_ptr=d_qof.ptr, reason_of_ptr=d_rof.ptr, stream=sp,
                               flags=G.EGRESS_MULTIBUF)
        wait()
        f.sync()
        np.testing.assert_array_equal(d_v.download(np.zeros(n, np.uint8))[:n_call], v[:n_call])
        cnt_h[:nports + 2 + M.REASONS] = m[2]
        np.testing.assert_array_equal(d_c.download(np.zeros_like(cnt_h)), cnt_h)
        qof_h[:n_call], rof_h[:n_call] = m[3], m[4]
        np.testing.assert_array_equal(d_qof.download(np.zeros_like(qof_h)), qof_h)
        np.testing.assert_array_equal(d_rof.download(np.zeros_like(rof_h)), rof_h)
        for q in range(nports + 1):
            tx_h[q][slots(E - 100 + q, len(m[0][q]), E - 1)] = m[0][q]
        fill_h[slots(0xfffffff0, len(m[1]), E - 1)] = m[1]
        np.testing.assert_array_equal(d_tx.download(np.zeros_like(tx_h)), tx_h)
        np.testing.assert_array_equal(d_fill.download(np.zeros_like(fill_h)), fill_h)
        np.testing.assert_array_equal(d_u.download(np.zeros_like(umem)), want_umem)
    finally:
        fib.free()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("where", ["library_stream", "caller_stream"])
def test_classify_frags_then_forward_without_sync(G, classified, where):  # noqa: F811
    import torch
    from test_gpu_steer_frags import frag_case
    n = len(classified[3])
    plens = np.concatenate([np.random.default_rng(5).integers(1, 6, n // 4), [n]])
    opts, v, done = frag_case(classified, plens)
    assert done < n and 0 < np.count_nonzero(v[:done] == PASS) < done
    stream = torch.cuda.Stream() if where == "caller_stream" else None
    sp = stream.cuda_stream if stream else None

    def classify(f, d_u, d_rx, d_flat, d_v):
        counts = f.classify_descs_frags(d_u.ptr, d_rx.ptr, n, d_v.ptr, stream=sp)
        return d_rx.ptr, counts[1], sp, torch.cuda.synchronize if sp else (lambda: None)

    composed(G, classified, opts, v, done, classify)


def test_forward_over_the_flat_array_of_classify_socks_frags(G, classified):  # noqa: F811
    """A poll round of a few SG sockets with trailing incomplete packets:
    sk->flat as a plain array, its VERDICT_NONE bytes keeping the sockets
    apart."""
    import steerfragmodel as F
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
    assert 0 < int((v == NONE).sum()) < n

    def classify(f, d_u, d_rx, d_flat, d_v):
        socks = [dict(rx_descs=d_rx.ptr + 16 * int(off[s]) if c else None, count=c, tx_descs=None,
                      fill_addrs=None) for s, c in enumerate(per)]
        f.classify_socks_frags(d_u.ptr, socks, d_v.ptr, flat_ptr=d_flat.ptr)
        return d_flat.ptr, n, None, lambda: None

    composed(G, classified, opts, v, n, classify)

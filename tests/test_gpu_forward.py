"""Forwarded egress (xfg_forward_egress, xfg_forward.hip): the PASS frames of
an RX batch to the TX ring of the egress port a device-resident FIB names,
their TTL, checksum and MACs rewritten in the UMEM; the PASS frames the program
would hand to the stack to the stack ring; the others' chunks to the fill ring.

Every comparison is exact against tests/fwdmodel.py, which
test_forward_reference.py holds equal to the reference's own xdp-forward
program run on the host (oracle/ref/ref_forward_harness.c) over a corpus and
100,000 mutated frames; test_gpu_forward_reference.py beside this file takes
its expected values from that run directly.  A case's frames are a pool of distinct
frames in a UMEM of random bytes and records that name each at most once;
every ring, queue_of, reason_of and counts are uploaded as 0xA5 bytes and
compared whole against a copy with the expected entries written in, and the
whole UMEM is compared, so a stray write shows.
"""
import numpy as np
import pytest

import fwdcorpus as K
import fwdmodel as M
from test_gpu_egress import A5, Rings, slots
from test_gpu_steer import umem_of_pool

pytestmark = pytest.mark.gpu

T, N3, verdicts_of = K.TILE, K.N3, K.verdicts_of


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


def run_forward(G, f, fib, pool, fid, v, routes, nexthops, ifx, kind="array", rot=0, fill=True,
                queue_of=True, reason_of=True, seed=3):
    """One call over the records fid (distinct indices into pool) with verdicts
    v over the ports ifx; everything compared with the model.  Returns the
    expected counts."""
    n = len(v)
    assert len(set(fid.tolist())) == n
    umem, paddr, pstart, plens = umem_of_pool(pool, seed)
    addr, lens, start = paddr[fid], plens[fid], pstart[fid]
    want_tx, want_fill, want_counts, want_qof, want_rof, after = M.forward_model(
        pool, fid, addr, lens, v, routes, nexthops, ifx)
    want_umem = umem.copy()
    for i in range(n):
        want_umem[start[i]:start[i] + len(after[i])] = np.frombuffer(after[i], np.uint8)
    return check_forward(G, f, fib, umem, addr, lens, v, ifx,
                         (want_tx, want_fill, want_counts, want_qof, want_rof, want_umem), kind=kind, rot=rot,
                         fill=fill, queue_of=queue_of, reason_of=reason_of)


def check_forward(G, f, fib, umem, addr, lens, v, ifx, want, kind="array", rot=0, fill=True, queue_of=True,
                  reason_of=True, options=True, classify=None):
    """One call over the records (addr, lens) with verdicts v over the ports
    ifx; checks counts, every ring, queue_of, reason_of and the UMEM whole
    against @want = (tx, fill, counts, queue_of, reason_of, umem): the first
    five as fwdmodel.forward_model returns them, the last the whole UMEM when
    the call has run, wherever they come from.  @classify(d_u, d_rx, d_v): the
    verdicts are not uploaded but left by what it launches, the forward call
    follows with nothing in between, and they must come out as v."""
    n, P = len(v), len(ifx)
    want_tx, want_fill, want_counts, want_qof, want_rof, want_umem = want
    rings = Rings(n, kind, rot)
    rx_e, tx_e, fill_e = rings.entries
    rx_h = np.full((max(rx_e, 1), 2), A5, np.uint64)
    rec = np.empty((n, 2), np.uint64)
    rec[:, 0] = addr
    rec[:, 1] = lens.astype(np.uint64)
    if options:     # option bits a TX record must not carry
        rec[:, 1] |= np.where(np.arange(n) % 5 == 4, 1 << 16, 0).astype(np.uint64) << np.uint64(32)
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
        if classify:
            d_v.upload(np.zeros(max(n, 16), np.uint8))
            f.sync()
            classify(d_u, d_rx, d_v)
        elif n:
            d_v.upload(np.ascontiguousarray(v))
        q_at = [(d_tx.ptr + q * tx_h[0].nbytes, tx_first[q], rings.mask[1]) for q in range(P + 1)]
        ports = [(ifx[q],) + q_at[q] for q in range(P)]
        f.forward_egress(d_u.ptr, d_rx.ptr, n, d_v.ptr, d_c.ptr, fib, ports, q_at[P],
                         fill_ptr=d_fill.ptr if fill else None, rx_first=rings.first[0],
                         rx_mask=rings.mask[0], fill_first=rings.first[2], fill_mask=rings.mask[2],
                         queue_of_ptr=d_qof.ptr if queue_of else None,
                         reason_of_ptr=d_rof.ptr if reason_of else None)
        f.sync()
        got = [d.download(np.zeros_like(a)) for d, a in zip(bufs, hosts)]
        if classify:
            np.testing.assert_array_equal(d_v.download(np.zeros(max(n, 16), np.uint8))[:n], v)
    finally:
        for b in bufs:
            b.free()
    got_umem, _, got_tx, got_fill, got_qof, got_rof, got_c = got
    cnt_h[:P + 2 + M.REASONS] = want_counts
    np.testing.assert_array_equal(got_c, cnt_h)
    assert int(want_counts[:P + 2].sum()) == n
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
    return want_counts


def case(G, f, fibs, nports, n, pattern="random", pool=None, **kw):
    routes, nexthops = K.fib_of(nports)
    pool = pool or K.pool_of(nports)
    fid = np.random.default_rng(100 + n + nports).permutation(len(pool))[:n]
    return run_forward(G, f, fibs(nports), pool, fid, verdicts_of(n, pattern), routes, nexthops,
                       K.ifindexes(nports), **kw)


# ---- 1: batch counts around the wave and the tile
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, N3])
def test_batch_counts(G, filt, fibs, n):
    case(G, filt, fibs, 8, n, kind=["array", "ring"][n % 2], rot=n)


# ---- 2: port counts, on three tiles
@pytest.mark.parametrize("nports", [1, 8, 63])
def test_port_counts(G, filt, fibs, nports):
    c = case(G, filt, fibs, nports, N3, kind="ring", rot=nports)
    assert (c[:nports + 1] > 0).all() and (c[nports + 2:] > 0).all()


# ---- 3: rings that wrap: the u32 index, the ring, a first past the mask, by turns
@pytest.mark.parametrize("rot", [0, 1, 2])
def test_rings_that_wrap(G, filt, fibs, rot):
    case(G, filt, fibs, 8, N3, kind="ring", rot=rot)


# ---- 4: verdict patterns
@pytest.mark.parametrize("pattern", ["no_pass", "all_pass"])
def test_no_pass_and_only_pass(G, filt, fibs, pattern):
    c = case(G, filt, fibs, 8, N3, pattern=pattern, kind="ring")
    assert c[9] == (N3 if pattern == "no_pass" else 0)


# ---- 5: one flow: a tile's 2048 records on one port (a slot's count 64, a prefix sum 1984)
def test_one_flow(G, filt, fibs):
    c = case(G, filt, fibs, 8, N3, pattern="all_pass", pool=K.one_flow_pool(), kind="ring", rot=1)
    assert sorted(c[:9].tolist())[-1] == N3 and c[10 + M.OK] == N3


# ---- 6: optional outputs
@pytest.mark.parametrize("given", [(False, True), (True, False), (False, False)])
def test_queue_of_and_reason_of_null(G, filt, fibs, given):
    case(G, filt, fibs, 8, N3, queue_of=given[0], reason_of=given[1])


def test_no_fill_ring(G, filt, fibs):
    case(G, filt, fibs, 8, N3, fill=False, kind="ring")


# ---- 7: the staging slots reused: the same FIB, another port table; two FIBs alive
def test_second_call_with_another_port_table(G, filt, fibs):
    """The FIB of the 8-port case, first over its own ports, then over ports
    in another order with one missing: its frames get NO_PORT."""
    routes, nexthops = K.fib_of(8)
    pool, fib = K.pool_of(8), fibs(8)
    ifx = K.ifindexes(8)
    fid = np.random.default_rng(5).permutation(len(pool))[:N3]
    v = verdicts_of(N3, "random", 1)
    a = run_forward(G, filt, fib, pool, fid, v, routes, nexthops, ifx, kind="ring")
    ifx2 = ifx[:0:-1]
    b = run_forward(G, filt, fib, pool, fid, v, routes, nexthops, ifx2, kind="ring", rot=2)
    assert b[7 + 2 + M.NO_PORT] > a[8 + 2 + M.NO_PORT]


def test_two_fibs_alive(G, filt, fibs):
    """Calls alternate between two FIBs with different routes and next hops."""
    fibs(8), fibs(63)
    for nports in (8, 63, 8):
        case(G, filt, fibs, nports, T + 1)

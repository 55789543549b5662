"""CPU tests of tests/fwdfragmodel.py, the model the GPU tests of
xfg_forward_frags_egress compare with: against fwdmodel.forward_model where
every record is its own packet, against a record-by-record walk, the packet
rules of the header comment, and -- where oracle/_ref/libref_forward.so is
built -- the heads' port, stage and bytes after against the reference's own
program.  Then the inputs of every GPU case (tests/test_gpu_forward_frags.py):
the condition a case is named for is asserted here, so no case quietly misses
its path."""
import numpy as np
import pytest

import fwdcorpus as K
import fwdfragmodel as W
import fwdmodel as M
import steerfragmodel as F
import xftools as X

PASS, NONE, T = W.PASS, W.NONE, W.T
NP = 8
ROUTES, NEXTHOPS = K.fib_of(NP)
IFX = K.ifindexes(NP)


def batch(n, seed, shape="random", none=0.0):
    rng = np.random.default_rng(seed)
    fid = rng.permutation(K.POOL)[:n]
    pool = W.pool_of(NP)
    lens = np.array([len(pool[k]) for k in fid], np.uint32)
    addr = (np.arange(n, dtype=np.uint64) * np.uint64(256)) | (np.uint64(16) << np.uint64(48))
    opts = F.opts_of_packet_lengths(W.plens_of(n, shape, seed), n) | (rng.integers(0, 2, n).astype(np.uint32) << 16)
    return pool, fid, addr, lens, opts, W.verdicts(n, seed, none)


def model(pool, fid, addr, lens, opts, v):
    return W.forward_frags_model(pool, fid, addr, lens, opts, v, ROUTES, NEXTHOPS, IFX)


def same(a, b, k=5):
    for x, y in zip(a[0], b[0]):
        np.testing.assert_array_equal(np.asarray(x, np.uint64).reshape(-1, 2), np.asarray(y, np.uint64).reshape(-1, 2))
    np.testing.assert_array_equal(np.asarray(a[1], np.uint64), np.asarray(b[1], np.uint64))
    for j in range(2, k):
        np.testing.assert_array_equal(np.asarray(a[j]).astype(np.uint64), np.asarray(b[j]).astype(np.uint64))


def after_of(pool, fid, m):
    return [m[6][int(k)][2] if ok else pool[k] for k, ok in zip(fid, m[5])]


def test_single_record_packets_equal_the_single_buffer_model():
    pool, fid, addr, lens, opts, v = batch(900, 1, "single")
    assert not (opts & F.CONTD).any() and (opts >> 16).any()
    got = model(pool, fid, addr, lens, opts, v)
    want = M.forward_model(pool, fid, addr, lens, v, ROUTES, NEXTHOPS, IFX)
    same(got, want)
    assert after_of(pool, fid, got) == list(want[5]) and got[5].sum() > 100


@pytest.mark.parametrize("none", [0.0, 0.1])
@pytest.mark.parametrize("shape", ["single", "three", "random"])
def test_model_equals_the_walk(shape, none):
    pool, fid, addr, lens, opts, v = batch(900, 2, shape, none)
    got = model(pool, fid, addr, lens, opts, v)
    want = W.walk([pool[k] for k in fid], addr, lens, opts, v, ROUTES, NEXTHOPS, IFX)
    same(got, want)
    assert after_of(pool, fid, got) == want[5]
    assert int(got[2][:NP + 2].sum()) == int((v != NONE).sum())


def test_a_packets_records_are_adjacent_and_in_order_on_one_ring():
    pool, fid, addr, lens, opts, v = batch(1500, 4, "random", 0.05)
    tx, fill, counts, qof, rof, ok, per = model(pool, fid, addr, lens, opts, v)
    live, head, head_of = F.packets(v, opts)
    where = {int(a): (q, k) for q in range(NP + 1) for k, a in enumerate(tx[q][:, 0].tolist())}
    seen = 0
    for h in np.flatnonzero(head):
        recs = np.flatnonzero(head_of == h)
        assert (np.diff(recs) == 1).all()
        if v[h] != PASS:
            assert (qof[recs] == W.QUEUE_NONE).all() and (rof[recs] == W.QUEUE_NONE).all()
            continue
        q0, k0 = where[int(addr[h])]
        assert [where[int(addr[r])] for r in recs] == [(q0, k0 + j) for j in range(len(recs))]
        assert (rof[recs] == rof[h]).all() and (q0 < NP) == (rof[h] == M.OK)
        np.testing.assert_array_equal(tx[q0][k0:k0 + len(recs), 1] >> np.uint64(32), opts[recs] & F.CONTD)
        seen += len(recs)
    assert seen == int(counts[:NP + 1].sum()) > 300
    assert (qof[~live] == W.QUEUE_NONE).all() and (rof[~live] == W.QUEUE_NONE).all()
    # the reasons count packets, the rings records
    assert int(counts[NP + 2:].sum()) == int((head & (v == PASS)).sum()) < seen


def test_continuation_bytes_and_verdicts_never_matter_and_only_heads_change():
    pool, fid, addr, lens, opts, v = batch(1200, 5, "random", 0.05)
    live, head, _ = F.packets(v, opts)
    want = model(pool, fid, addr, lens, opts, v)
    rng = np.random.default_rng(6)
    cont = live & ~head
    assert cont.sum() > 500
    fid2, v2 = fid.copy(), v.copy()
    fid2[cont] = rng.integers(0, K.POOL, int(cont.sum()))
    v2[cont] = rng.integers(0, 5, int(cont.sum()))              # anything but VERDICT_NONE
    got = model(pool, fid2, addr, lens, opts, v2)
    same(got, want)
    np.testing.assert_array_equal(got[5], want[5])
    assert not want[5][~head].any() and not want[5][v != PASS].any()      # only PASS heads are rewritten
    k = int(np.flatnonzero(cont)[10])
    v3 = v.copy()
    v3[k] = NONE            # ... unless the byte is VERDICT_NONE: the packet ends there
    got = model(pool, fid, addr, lens, opts, v3)
    assert got[3][k] == W.QUEUE_NONE and int(got[2][:NP + 2].sum()) == int(want[2][:NP + 2].sum()) - 1


def test_applied_twice_the_model_decrements_twice():
    pool, fid, addr, lens, opts, v = batch(600, 7, "three")
    m1 = model(pool, fid, addr, lens, opts, v)
    frames1 = after_of(pool, fid, m1)
    m2 = model(frames1, np.arange(600), addr, lens, opts, v)
    h = np.flatnonzero(m1[5] & m2[5])
    assert len(h) > 50
    for i in h[:50]:
        l3 = M.parse_ethhdr(pool[fid[i]])[1]
        assert m2[6][int(i)][2][l3 + 8] == pool[fid[i]][l3 + 8] - 2
    gone = np.flatnonzero(m1[5] & ~m2[5])           # TTL 2 at first: forwarded once, then XFG_FWD_TTL
    assert all(pool[fid[i]][M.parse_ethhdr(pool[fid[i]])[1] + 8] == 2 for i in gone)
    assert (m2[4][gone] == M.TTL).all()


def test_heads_equal_the_reference():
    """The fwdrefcorpus frames as heads, each followed by 0-3 continuation
    records holding other corpus frames: port, stage and bytes after of every
    PASS packet are what the reference's program gives the head buffer."""
    if not X.have_reference_forward():
        pytest.skip("oracle/_ref/libref_forward.so is not built")
    import fwdrefcorpus as R
    data, lens = R.slots()
    n = len(lens)
    table = 8
    ifx = R.ifindexes(table)
    rq, stage, after, _ = X.run_reference_forward(data.reshape(-1), lens, R.routes(), R.nexthops(table), ifx,
                                                  stride=data.shape[1])
    pool = [data[i, :lens[i]].tobytes() for i in range(n)]
    rng = np.random.default_rng(11)
    extra = rng.integers(0, 4, n)
    heads = np.concatenate([[0], np.cumsum(extra + 1)[:-1]])
    total = int((extra + 1).sum())
    fid = rng.integers(0, n, total)
    fid[heads] = np.arange(n)
    opts = F.opts_of_packet_lengths(extra + 1, total)
    nh = [tuple(x) for x in R.nexthops(table)]
    got = W.forward_frags_model(pool, fid, np.arange(total) * 256, lens[fid], opts, np.full(total, PASS, np.uint8),
                                [tuple(r) for r in R.routes()], nh, ifx)
    np.testing.assert_array_equal(got[3], np.repeat(rq, extra + 1).astype(np.uint8))
    np.testing.assert_array_equal(got[5][heads], stage == X.FWD_ST_REDIRECT)
    np.testing.assert_array_equal(got[4][heads] == M.OK, stage == X.FWD_ST_REDIRECT)
    w = after.shape[1]
    for i in np.flatnonzero(got[5][heads]):
        g = np.frombuffer(got[6][int(i)][2], np.uint8)[:w]
        np.testing.assert_array_equal(g, after[i, :len(g)])


# ---- the GPU cases' inputs
def case_model(nports, fid, opts, v):
    routes, nexthops = K.fib_of(nports)
    n = len(v)
    return W.forward_frags_model(W.pool_of(nports), fid, np.arange(n, dtype=np.uint64) * 128,
                                 W.pool_matrix(nports)[1][fid], opts, v, routes, nexthops, K.ifindexes(nports))


def test_special_frames_are_routable_but_for_their_ttl():
    pool = W.pool_of(NP)
    look = lambda d: M.lpm(ROUTES, d)       # noqa: E731
    for k in range(W.NSPECIAL):
        r, q, g = M.forward_frame(pool[W.TTL2 + k], look, NEXTHOPS, IFX)
        assert r == M.OK and q is not None and g[22] == 1
        assert M.forward_frame(pool[W.TTL1 + k], look, NEXTHOPS, IFX)[0] == M.TTL
        assert M.forward_frame(g, look, NEXTHOPS, IFX)[0] == M.TTL      # what a second look would say
    assert W.NSPECIAL >= W.HAZARD_TILES - 1 and max(map(len, pool)) <= 96


@pytest.mark.parametrize("ttl", [2, 1])
def test_hazard_case_straddles_every_boundary(ttl):
    fid, opts, v, heads = W.hazard(ttl)
    live, head, head_of = F.packets(v, opts)
    straddling = [h for h in heads if head[h] and v[h] == PASS and head_of[h + 4] == h and h // T != (h + 4) // T
                  and (fid[h] >= W.TTL2) and (fid[h] < W.TTL1) == (ttl == 2)]
    assert len(straddling) >= W.HAZARD_TILES - 1
    m = case_model(8, fid, opts, v)
    for d in range(5):
        assert (m[4][heads + d] == (M.OK if ttl == 2 else M.TTL)).all()
        assert ((m[3][heads + d] < 8) if ttl == 2 else (m[3][heads + d] == 8)).all()
    assert m[5][heads].all() == (ttl == 2)


@pytest.mark.parametrize("name", list(W.PLACEMENTS))
def test_placement_cases(name):
    first, n = W.PLACEMENTS[name]
    for headv in ("pass", "other"):
        fid, opts, v, h = W.placement(name, headv)
        live, head, head_of = F.packets(v, opts)
        assert head[h] and int((head_of == h).sum()) == first[-1]
        assert h // T != (h + first[-1] - 1) // T or name in ("tile_edges", "wave_last_lane")
    if name == "tile_edges":
        assert h == T and (opts[T - 1] & 1) == 0
    if name == "head_on_tile_last":
        assert h == T - 1
    if name == "wave_last_lane":
        assert h % 64 == 63
    if name == "straddle_70":
        assert T - h == 67
    if name == "two_tiles_and_3":
        assert not head[T:2 * T].any() and live[T:2 * T].all()      # a tile with no head
        fid, opts, v, h = W.placement(name, "pass", ttl=2)
        m = case_model(8, fid, opts, v)
        assert (m[4][h:h + 2 * T + 3] == M.OK).all()


@pytest.mark.parametrize("where", list(W.NONE_RUNS))
def test_none_run_cases(where):
    fid, opts, v = W.none_runs(where)
    live, head, _ = F.packets(v, opts)
    n = len(v)
    if where == "all":
        assert not live.any()
    else:
        # a packet cut by a run: the record behind the run is a head though its predecessor goes on
        assert any(b < n and live[b] and head[b] and (opts[b - 1] & F.CONTD) for _, b in W.NONE_RUNS[where])


def test_every_reason_port_and_the_stack_ring_by_packets_of_several_records():
    fid, opts, v = W.every_reason()
    m = case_model(8, fid, opts, v)
    live, head, head_of = F.packets(v, opts)
    multi = np.flatnonzero(head & (v == PASS) & np.r_[(opts[:-1] & 1) != 0, False])
    assert set(m[4][multi].tolist()) == set(range(M.REASONS))
    assert set(m[3][multi].tolist()) == set(range(9))
    for nports in W.PORTS:
        n = W.N3
        reached = np.zeros(nports + 2, bool)
        for shape in W.SHAPES:      # (test_partition's batches of three tiles)
            k = 3 + W.PORTS.index(nports) + W.SHAPES.index(shape)
            m = case_model(nports, W.fids(n), W.option_words(W.plens_of(n, shape), n),
                           W.verdicts(n, k, 0.0 if shape == "single" else 0.03))
            reached |= m[2][:nports + 2] > 0
            assert (m[2][:nports + 2] > 0).sum() >= min(nports, 56) + 2
        assert reached.all()


def test_continuations_would_go_elsewhere():
    n = W.N3
    fid, opts, v = W.fids(n, 5), W.option_words(W.plens_of(n, "random", 5), n), W.verdicts(n, 5)
    live, head, head_of = F.packets(v, opts)
    cont = np.flatnonzero(live & ~head)
    assert len(cont) > n // 2 and np.mean(v[cont] != v[head_of[cont]]) > 0.3
    own = case_model(63, fid, np.zeros(n, np.uint32), np.full(n, PASS, np.uint8))
    pkt = case_model(63, fid, opts, np.full(n, PASS, np.uint8))
    routable = own[4][cont] == M.OK
    assert routable.mean() > 0.3 and np.mean(own[3][cont][routable] != pkt[3][cont][routable]) > 0.8

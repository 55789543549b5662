"""CPU tests of tests/steerfragmodel.py, the model the GPU tests of
xfg_steer_frags_egress compare with: against steermodel.steer_model where every
record is its own packet, against a record-by-record walk, the packet rules of
the header comment, and -- where oracle/_ref/libref_cpumap.so is built -- the
head queues against the reference's own programs on the head buffers."""
import numpy as np
import pytest

import steercorpus as S
import steerfragmodel as F
import steermodel as M
import xftools as X

PASS, NONE = F.PASS, F.VERDICT_NONE
OTHERS = np.array([0, 1, 3, 4], np.uint8)


def pool():
    return [f for _, f in M.hand_rows()] + [f for f in S.corpus().frames[::97]]


def batch(n, seed, shape="random", none=0.0):
    """n records naming pool frames, cut into packets; 60 % of the bytes PASS."""
    rng = np.random.default_rng(seed)
    P = pool()
    fid = rng.integers(0, len(P), n)
    lens = np.array([len(P[k]) for k in fid], np.uint32)
    addr = (np.arange(n, dtype=np.uint64) * np.uint64(256)) | (np.uint64(16) << np.uint64(48))
    v = OTHERS[rng.integers(0, len(OTHERS), n)]
    v[rng.random(n) < 0.6] = PASS
    v[rng.random(n) < none] = NONE
    plens = {"single": np.ones(n, np.int64), "three": np.full(n, 3),
             "random": rng.integers(1, 19, n)}[shape]
    opts = F.opts_of_packet_lengths(plens, n) | (rng.integers(0, 2, n).astype(np.uint32) << 16)
    return P, fid, addr, lens, opts, v


def same(a, b):
    for x, y in zip(a[0], b[0]):
        np.testing.assert_array_equal(np.asarray(x, np.uint64).reshape(-1, 2), np.asarray(y, np.uint64).reshape(-1, 2))
    np.testing.assert_array_equal(np.asarray(a[1], np.uint64), np.asarray(b[1], np.uint64))
    np.testing.assert_array_equal(np.asarray(a[2], np.uint64), np.asarray(b[2], np.uint64))
    np.testing.assert_array_equal(np.asarray(a[3], np.uint8), np.asarray(b[3], np.uint8))


@pytest.mark.parametrize("mode", [M.L4_HASH, M.L4_SPORT, M.L4_DPORT])
@pytest.mark.parametrize("nq", [1, 7, 64])
def test_single_record_packets_equal_the_single_buffer_model(nq, mode):
    P, fid, addr, lens, opts, v = batch(700, 1, "single")
    assert not (opts & F.CONTD).any() and (opts >> 16).any()
    got = F.steer_frags_model(P, addr, lens, opts, v, nq, mode, None, nq - 1, fid=fid)
    want = M.steer_model(P, addr, lens, v, nq, mode, None, nq - 1, fid=fid)
    same(got, want)
    assert got[2][nq + 1] > 0


@pytest.mark.parametrize("none", [0.0, 0.1])
@pytest.mark.parametrize("shape", ["single", "three", "random"])
def test_model_equals_the_walk(shape, none):
    P, fid, addr, lens, opts, v = batch(900, 2, shape, none)
    avail = np.random.default_rng(3).integers(0, 5, 256).tolist()
    for mode in (M.L4_HASH, M.L4_DPORT):
        got = F.steer_frags_model(P, addr, lens, opts, v, 5, mode, avail, 2, fid=fid)
        want = F.walk([P[k] for k in fid], addr, lens, opts, v, 5, mode, avail, 2)
        same(got, want)
        live = int((v != NONE).sum())
        assert int(got[2][:6].sum()) == live


def test_packet_rules():
    #           h  c  e  |h e| N |h(open run) N | h c(e)
    v = np.array([2, 0, 9, 1, NONE, 2, 2, NONE, 3, 2], np.uint8)
    o = np.array([1, 1, 0, 0, 1, 1, 1, 0, 1, 0], np.uint32)
    live, head, head_of = F.packets(v, o)
    assert live.tolist() == [1, 1, 1, 1, 0, 1, 1, 0, 1, 1]
    assert head.tolist() == [1, 0, 0, 1, 0, 1, 0, 0, 1, 0]
    assert head_of.tolist() == [0, 0, 0, 3, -1, 5, 5, -1, 8, 8]


def test_a_packets_records_are_adjacent_and_in_order_on_one_ring():
    P, fid, addr, lens, opts, v = batch(1500, 4, "random", 0.05)
    tx, fill, counts, qof = F.steer_frags_model(P, addr, lens, opts, v, 7, fid=fid)
    live, head, head_of = F.packets(v, opts)
    where = {}
    for q in range(7):
        for k, a in enumerate(tx[q][:, 0].tolist()):
            where[a] = (q, k)
    assert len(where) == int(counts[:7].sum())
    seen = 0
    for h in np.flatnonzero(head):
        recs = np.flatnonzero(head_of == h)
        assert (np.diff(recs) == 1).all()                       # a run of records
        if v[h] != PASS:
            assert (qof[recs] == F.QUEUE_NONE).all()
            continue
        q0, k0 = where[int(addr[h])]
        assert [where[int(addr[r])] for r in recs] == [(q0, k0 + j) for j in range(len(recs))]
        # XDP_PKT_CONTD as received: set on all but a complete packet's last record
        np.testing.assert_array_equal(tx[q0][k0:k0 + len(recs), 1] >> np.uint64(32), opts[recs] & F.CONTD)
        seen += len(recs)
    assert seen == int(counts[:7].sum()) > 300
    assert (qof[~live] == F.QUEUE_NONE).all()


def test_continuation_bytes_and_verdicts_never_matter():
    P, fid, addr, lens, opts, v = batch(1200, 5, "random", 0.05)
    live, head, _ = F.packets(v, opts)
    want = F.steer_frags_model(P, addr, lens, opts, v, 7, M.L4_SPORT, fid=fid)
    rng = np.random.default_rng(6)
    cont = live & ~head
    assert cont.sum() > 500
    fid2, v2 = fid.copy(), v.copy()
    fid2[cont] = rng.integers(0, len(P), int(cont.sum()))
    v2[cont] = rng.integers(0, 5, int(cont.sum()))              # anything but VERDICT_NONE
    # (lens and addr are the record's own and stay: they are copied to the ring)
    same(F.steer_frags_model(P, addr, lens, opts, v2, 7, M.L4_SPORT, fid=fid2), want)
    # ... unless the byte is VERDICT_NONE: the packet ends there, the next live record is a head
    k = int(np.flatnonzero(cont)[10])
    v3 = v.copy()
    v3[k] = NONE
    got = F.steer_frags_model(P, addr, lens, opts, v3, 7, M.L4_SPORT, fid=fid)
    assert got[3][k] == F.QUEUE_NONE and int(got[2][:8].sum()) == int(want[2][:8].sum()) - 1


def test_refused_heads_count_per_packet():
    short = M.eth(M.ETH_P_IP, b"")[:13]
    frames = [short] * 6
    v = np.full(6, PASS, np.uint8)
    o = np.array([1, 1, 0, 1, 0, 0], np.uint32)
    tx, fill, counts, qof = F.steer_frags_model(frames, np.arange(6) * 64, np.full(6, 13), o, v, 4,
                                                skip_queue=3)
    assert counts.tolist() == [0, 0, 0, 6, 0, 3] and qof.tolist() == [3] * 6


def test_head_queues_equal_the_reference():
    """The corpus's frames as heads, each followed by 0-3 continuation records
    holding other corpus frames: the model's queue of every PASS packet is what
    the reference's program returns on the head buffer."""
    if not X.have_reference_steer():
        pytest.skip("oracle/_ref/libref_cpumap.so is not built")
    c = S.corpus()
    data, lens = S.slots()
    n = len(c.frames)
    cut = [fr[:int(k)] for fr, k in zip(c.frames, c.lens)]
    rng = np.random.default_rng(11)
    extra = rng.integers(0, 4, n)
    heads = np.concatenate([[0], np.cumsum(extra + 1)[:-1]])
    total = int((extra + 1).sum())
    fid = rng.integers(0, n, total)
    fid[heads] = np.arange(n)
    opts = F.opts_of_packet_lengths(extra + 1, total)
    v = np.full(total, PASS, np.uint8)
    for mode in (M.L4_HASH, M.L4_SPORT, M.L4_DPORT):
        for avail in (list(range(64)), list(range(7))):
            rq, rr = X.run_reference_steer(data.reshape(-1), lens, mode, avail, len(avail) - 1,
                                           stride=S.MAXLEN)
            got = F.steer_frags_model(cut, np.arange(total) * 256, c.lens[fid], opts, v, len(avail), mode,
                                      avail, len(avail) - 1, fid=fid)
            np.testing.assert_array_equal(got[3][heads], rq)
            np.testing.assert_array_equal(got[3], np.repeat(rq, extra + 1))
            assert int(got[2][len(avail) + 1]) == int(np.asarray(rr).sum())

"""tests/fwdmodel.py -- the model the GPU tests of xfg_forward_egress were first
written against -- and the corpus of tests/fwdrefcorpus.py against the
reference's own xdp-forward program, compiled for the host without
modification (oracle/ref/ref_forward_harness.c).  Whatever is
compared, the expected values come from the reference library alone; where the
two differ the reference is right on the return code, the redirect key and the
bytes, and include/xdpfilter_gpu.h on how XFG_FWD_* splits what the program
returns alike.  All comparisons are exact.

Skipped where the library was not built (no reference tree at build time); the
GPU file beside this one, test_gpu_forward_reference.py, fails instead.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import fwdcorpus as K
import fwdmodel as M
import fwdrefcorpus as F
import test_forward_model as H
import xftools as X

pytestmark = pytest.mark.skipif(not X.have_reference_forward(),
                                reason="oracle/_ref/libref_forward.so not built (no reference tree)")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFUZZ = 100_000
Q, AD = M.ETH_P_8021Q, M.ETH_P_8021AD
# fwdmodel's reason -> the stages the reference may report for it
STAGES_OF_REASON = {M.OK: {5}, M.NO_ROUTE: {1}, M.NH_RET: {2}, M.FRAG: {3}, M.NO_PORT: {4},
                    M.NOT_IP: {0}, M.BAD_HDR: {0}, M.TTL: {0}, M.V6: {0, 6}}


def reference(data, lens, routes, nexthops, ports, mode=X.FWD_FULL):
    return X.run_reference_forward(data.reshape(-1), lens, routes, nexthops, ports, stride=data.shape[1],
                                   mode=mode)


def model(data, lens, routes, nexthops, ports):
    """(reason, queue, after) of fwdmodel.forward_frame, frame by frame."""
    memo = {}

    def lookup(dst):
        if dst not in memo:
            memo[dst] = M.lpm(routes, dst)
        return memo[dst]

    n = len(lens)
    reason, queue = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    after = np.zeros((n, max(int(lens.max()), 1)), np.uint8)
    for i in range(n):
        r, q, g = M.forward_frame(data[i, :lens[i]].tobytes(), lookup, nexthops, ports)
        reason[i], queue[i] = r, len(ports) if q is None else q
        after[i, :len(g)] = np.frombuffer(g, np.uint8)
    return reason, queue, after


def agree(data, lens, got, want):
    """The model's (reason, queue, after) against the reference's (queue,
    stage, after, seen): the queue (so the return code and the key), the bytes,
    and the reason against the stage."""
    reason, queue, after = got
    rq, stage, rafter, _ = want
    ok = np.array([int(s) in STAGES_OF_REASON[int(r)] for r, s in zip(reason, stage)])
    bad = np.flatnonzero((queue != rq) | (after[:, :rafter.shape[1]] != rafter).any(axis=1) | ~ok)
    out = [f"{len(bad)} of {len(lens)} frames differ"]
    for i in bad[:6].tolist():
        out.append(f"frame {i} len {lens[i]} model {M.REASON_NAMES[reason[i]], int(queue[i])} reference stage "
                   f"{int(stage[i])} queue {int(rq[i])}: {data[i, :lens[i]].tobytes().hex()} -> "
                   f"{after[i, :lens[i]].tobytes().hex()} / {rafter[i, :lens[i]].tobytes().hex()}")
    assert not len(bad), "\n".join(out)


@functools.lru_cache(maxsize=None)
def corpus_reference(table, mode=X.FWD_FULL):
    data, lens = F.slots()
    return reference(data, lens, F.routes(), F.nexthops(table), F.ifindexes(table), mode)


# ---- the model equals the reference
@pytest.mark.parametrize("table", F.TABLES)
def test_model_on_corpus(table):
    data, lens = F.slots()
    got = model(data, lens, F.routes(), F.nexthops(table), F.ifindexes(table))
    agree(data, lens, got, corpus_reference(table))
    # the split within stage 0, and V6 over stages 0 and 6, is the tag's
    c = F.corpus()
    stage = corpus_reference(table)[1]
    for i in range(len(lens)):
        tag = F.TAGS[c.tag[i]]
        want = F.REASON_OF[tag] if tag != "lookup" else F.REASON_OF_STAGE[int(stage[i])]
        assert got[0][i] == want, (i, tag, M.REASON_NAMES[got[0][i]], c.frames[i].hex())


@functools.lru_cache(maxsize=None)
def mutated():
    """NFUZZ corpus frames with one to three bytes changed in the first 54 (half
    of the new values from a list of meaningful ones) and a cut at a random
    length 0 .. len (so one in len + 1 stays whole)."""
    data, lens = F.slots()
    rng = np.random.default_rng(7200)
    pick = rng.integers(0, len(lens), NFUZZ)
    out, olens = data[pick].copy(), lens[pick].copy()
    special = np.array([0, 1, 2, 0x08, 0x45, 0x46, 0x4f, 0x40, 0x60, 0x81, 0x88, 0xa8, 0x86, 0xdd, 0xfe, 0xff,
                        0x0a, 0x14, 0xc0, 0xac, 0x2c], np.uint8)
    rows = np.arange(NFUZZ)
    for k in range(3):
        on = rng.random(NFUZZ) < (1.0, 0.5, 0.25)[k]
        at = rng.integers(0, 54, NFUZZ)
        val = np.where(rng.random(NFUZZ) < 0.5, special[rng.integers(0, len(special), NFUZZ)],
                       rng.integers(0, 256, NFUZZ)).astype(np.uint8)
        on &= at < olens
        out[rows[on], at[on]] = val[on]
    olens = np.minimum((rng.random(NFUZZ) * (olens + 1)).astype(np.uint32), olens)
    out[np.arange(F.MAXLEN)[None, :] >= olens[:, None]] = 0
    out.setflags(write=False)
    olens.setflags(write=False)
    return out, olens


@pytest.mark.parametrize("table", [8, "collide"])
def test_model_on_mutated_frames(table):
    data, lens = mutated()
    routes, nexthops, ports = F.routes(), F.nexthops(table), F.ifindexes(table)
    want = reference(data, lens, routes, nexthops, ports)
    agree(data, lens, model(data, lens, routes, nexthops, ports), want)
    hist = np.bincount(want[1], minlength=X.FWD_STAGES)
    print("stages of the mutated frames:", hist.tolist())
    assert (hist >= 100).all()


@pytest.mark.parametrize("table", F.TABLES)
def test_direct_answers_as_full(table):
    """BPF_FIB_LOOKUP_DIRECT reaches only the lookup's stand-in."""
    a, b = corpus_reference(table), corpus_reference(table, X.FWD_DIRECT)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ---- the hand rows of test_forward_model.py, recomputed through the reference
def through_reference(frames):
    """(reason-compatible stage, queue or None, bytes after) per frame over
    test_forward_model.py's routes, next hops and ports."""
    data = np.zeros((len(frames), max(max(map(len, frames)), 1)), np.uint8)
    for i, f in enumerate(frames):
        data[i, :len(f)] = np.frombuffer(f, np.uint8)
    lens = np.array([len(f) for f in frames], np.uint32)
    q, stage, after, _ = reference(data, lens, H.ROUTES, H.NEXTHOPS, H.PORTS)
    return [(int(stage[i]), None if q[i] == len(H.PORTS) else int(q[i]), after[i, :lens[i]].tobytes())
            for i in range(len(frames))]


def test_every_reason_by_hand():
    v4 = H.v4
    rows = [(v4(), M.OK, 1),
            (b"\x00" * 13, M.NOT_IP, None),
            (M.eth(M.ETH_P_ARP, bytes(28)), M.NOT_IP, None),
            (v4()[:33], M.BAD_HDR, None),
            (v4(ttl=1), M.TTL, None),
            (v4(ttl=0), M.TTL, None),
            (M.eth(M.ETH_P_IPV6, bytes(40)), M.V6, None),
            (M.eth(M.ETH_P_IPV6, b""), M.V6, None),
            (M.eth(M.ETH_P_IPV6, bytes([0x60, 0, 0, 0, 0, 8, 17, 64]) + bytes(40)), M.V6, None),
            (v4(M.ip_bytes(0x0e000001)), M.NO_ROUTE, None),
            (v4(M.ip_bytes(0x0b000001)), M.NH_RET, None),
            (v4(M.ip_bytes(0x0c000001), tot_len=101), M.FRAG, None),
            (v4(M.ip_bytes(0x0c000001), tot_len=100), M.OK, 0),
            (v4(M.ip_bytes(0x0c000001), payload=bytes(76), tot_len=20), M.OK, 0),
            (v4(M.ip_bytes(0x0d000001)), M.NO_PORT, None)]
    got = through_reference([f for f, _, _ in rows])
    for (f, reason, q), (stage, gq, g) in zip(rows, got):
        assert stage in STAGES_OF_REASON[reason] and gq == q, (f.hex(), M.REASON_NAMES[reason], stage, gq)
        assert H.fwd(f)[:2] == (reason, q) and H.fwd(f)[2] == g
        if reason != M.OK:
            assert g == f
    # the IPv6 rows' stages: hop_limit 0, no header, a whole header
    assert [s for s, _, _ in got[6:9]] == [0, 0, 6]


def test_ihl_against_len():
    frames, want = [], []
    for ihl in range(16):
        f = H.v4(ihl=ihl, payload=bytes(8))
        frames += [f[:14 + 4 * max(ihl, 5)], f[:14 + max(20, 4 * ihl) - 1]]
        want += [5, 0]
        if ihl < 5:
            frames += [f[:14 + 20], f[:14 + 19]]
            want += [5, 0]
    got = through_reference(frames)
    assert [s for s, _, _ in got] == want
    for f, (s, q, g) in zip(frames, got):
        assert H.fwd(f)[1:] == (q, g)


def test_a_tag_cut_at_every_length():
    frames, want, reasons = [], [], []
    for ntags in (1, 2, 3, 4):
        f = H.v4(tags=(Q,) * ntags)
        frames += [f[:14 + 4 * (ntags - 1) + cut] for cut in range(4)] + [f[:14 + 4 * ntags], f]
        want += [0] * 5 + [5]
        reasons += [M.NOT_IP] * 4 + [M.BAD_HDR, M.OK]
    got = through_reference(frames)
    assert [s for s, _, _ in got] == want
    for f, r, (s, q, g) in zip(frames, reasons, got):
        assert H.fwd(f) == (r, q, g)


def test_tag_counts():
    frames = [H.v4(tags=tuple([AD, Q][k % 2] for k in range(ntags))) for ntags in range(6)]
    got = through_reference(frames)
    for ntags, (f, (s, q, g)) in enumerate(zip(frames, got)):
        if ntags <= 4:
            l3 = 14 + 4 * ntags
            assert (s, q) == (5, 1)
            assert g[12:l3] == f[12:l3] and g[l3 + 8] == f[l3 + 8] - 1
            assert g[:12] == H.NEXTHOPS[0][3] + H.NEXTHOPS[0][4]
        else:
            assert (s, q, g) == (0, None, f)
        assert H.fwd(f)[1:] == (q, g)


# ---- the check field: all 65,536 stored values
# A header that was valid and is not after ip_decrease_ttl(), by stored value
# as the little-endian load sees it.  None: where the step's sum passes 0xFFFF
# it adds the carry back in, and where it lands on 0xFFFF it stores 0x0000, the
# other zero of ones' complement arithmetic, which sums alike.
CHECK_EXCEPTIONS = ()


def test_every_check_value():
    data, lens = F.check_slots()
    routes, nexthops, ports = F.routes(), F.nexthops(8), F.ifindexes(8)
    want = reference(data, lens, routes, nexthops, ports)
    assert (want[1] == X.FWD_ST_REDIRECT).all()
    agree(data, lens, model(data, lens, routes, nexthops, ports), want)
    k = np.arange(F.NCHECK)
    l3 = 14 + 4 * (k % 5)
    cols = l3[:, None] + np.arange(20)

    def csum(a):
        """csum16 of every row's header: the sum from scratch."""
        h = np.take_along_axis(a, cols, axis=1)
        s = (h[:, 0::2].astype(np.uint32) << 8 | h[:, 1::2]).sum(axis=1)
        s = (s & 0xffff) + (s >> 16)
        return (s & 0xffff) + (s >> 16)

    before, after = data[:, :want[2].shape[1]], want[2]
    assert M.csum16(before[0, 14:34].tobytes()) == csum(before)[0] == 0xFFFF      # the two sums agree
    assert (csum(before) == 0xFFFF).all()
    stored = before[k, l3 + 10].astype(np.uint32) | before[k, l3 + 11].astype(np.uint32) << 8
    assert np.array_equal(stored, k)
    broken = np.flatnonzero(csum(after) != 0xFFFF)
    assert tuple(broken.tolist()) == CHECK_EXCEPTIONS
    assert np.array_equal(after[k, l3 + 8], before[k, l3 + 8] - 1)
    new = after[k, l3 + 10].astype(np.uint32) | after[k, l3 + 11].astype(np.uint32) << 8
    assert new[0xFFFE] == 0x0000 and new[0xFFFF] == 0x0001 and new[0x0000] == 0x0001 and new[0xFEFF] == 0xFF00


# ---- what the program handed the lookup
def l3_of(f):
    at = 14
    while f[at - 2:at] in (b"\x81\x00", b"\x88\xa8") and at < 30:
        at += 4
    return at


@pytest.mark.parametrize("table", [8, "collide"])
def test_lookup_inputs(table):
    c = F.corpus()
    _, stage, _, seen = corpus_reference(table)
    called = 0
    for i, f in enumerate(c.frames):
        if stage[i] == 0:
            assert seen[i].tolist() == [0xffffffff] * 3
            continue
        called += 1
        l3 = l3_of(f)
        if stage[i] == 6:
            assert seen[i, :2].tolist() == [10, int.from_bytes(f[l3 + 4:l3 + 6], "big")]
        else:
            assert seen[i].tolist() == [2, int.from_bytes(f[l3 + 2:l3 + 4], "big"),
                                        int.from_bytes(f[l3 + 16:l3 + 20], "little")]
    assert called > 4000


# ---- the corpus cannot quietly turn bland
def test_corpus_shape():
    c = F.corpus()
    n = len(c.frames)
    assert n > 4 * F.TILE and n % F.TILE and max(map(len, c.frames)) <= F.MAXLEN
    assert set(np.unique(c.part)) == set(range(len(F.PARTS)))
    assert {14, 17, 18, 33, 34} <= set(c.lens[c.part == F.PARTS.index("short")].tolist())
    ports, a, b = F.colliding()
    assert len(set(ports)) == 63 and {F.fwd_hash(i) for i in ports} == {126, 127}
    assert a not in ports and b not in ports and F.fwd_hash(a) == 126 and F.fwd_hash(b) == 100
    dist = F.probe_distances(ports)
    assert max(dist) >= 60 and sorted((F.fwd_hash(i) + d) % 128 for i, d in zip(ports, dist)) == \
        sorted([126, 127] + list(range(61)))


@pytest.mark.parametrize("tag", [t for t in F.TAGS])
def test_every_return_statement_is_reached(tag):
    c = F.corpus()
    sel = c.tag == F.TAGS.index(tag)
    assert sel.sum() >= 8
    for table in F.TABLES:
        q, stage, _, _ = corpus_reference(table)
        assert set(np.unique(stage[sel]).tolist()) <= F.STAGES_OF[tag]
        assert ((q[sel] < len(F.ifindexes(table))) == (stage[sel] == 5)).all()


@pytest.mark.parametrize("table", F.TABLES)
def test_corpus_conditions(table):
    """From the reference's answers alone, under the GPU tests' verdicts: a
    permutation of the corpus with about 60 % PASS."""
    fid, v = F.permuted()
    ifx = F.ifindexes(table)
    P = len(ifx)
    q, stage, _, seen = corpus_reference(table)
    passed = v == M.PASS
    q, stage, seen = q[fid][passed], stage[fid][passed], seen[fid][passed]
    hist = np.bincount(stage, minlength=X.FWD_STAGES)
    per = np.bincount(q, minlength=P + 1)
    print(f"table {table}: stages {hist.tolist()}, fewest a port {per[:P].min()}, stack ring {per[P]}")
    assert (hist >= 50).all()
    assert len(per) == P + 1 and (per > 0).all()
    assert 0.30 <= hist[5] / passed.sum() <= 0.70
    # a /24 with a longer prefix in it resolves through its second-level group
    deep24 = np.array(sorted({p >> 8 for p, l, _ in F.routes() if l > 24}), np.uint32)
    dst24 = seen[stage == 5][:, 2].astype(np.uint32).byteswap() >> 8
    deep = int(np.isin(dst24, deep24).sum())
    print(f"  forwarded through a group {deep}, without {len(dst24) - deep}")
    assert deep >= 50 and len(dst24) - deep >= 50
    if table == "collide":
        dist = np.array(F.probe_distances(ifx))
        far = int((dist[q[stage == 5]] >= 40).sum())
        _, a, b = F.colliding()
        on_a = (seen[:, 2].astype(np.uint32).byteswap() >> 16) == (F.NET_ABSENT_A >> 16)
        on_b = (seen[:, 2].astype(np.uint32).byteswap() >> 16) == (F.NET_ABSENT_B >> 16)
        print(f"  forwarded to a port 40 probes or more from home {far}; absent in slot 126 {on_a.sum()}, "
              f"in an empty slot {on_b.sum()}")
        assert far >= 50
        assert on_a.sum() >= 20 and (stage[on_a] == 4).all()
        assert on_b.sum() >= 20 and (stage[on_b] == 4).all()


# ---- the harness under ASAN + UBSAN, in a program of its own
@pytest.fixture(scope="module")
def harness_program(tmp_path_factory):
    """oracle/_ref/ref_forward_asan, built here by `make -C oracle ref-asan`
    (the harness with its own main).  Skipped only where the C compiler has no
    ASAN/UBSAN runtime that runs, or there is no reference tree to compile."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    d = tmp_path_factory.mktemp("ref_forward_asan")
    probe = d / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run([cc, *san, "-o", str(d / "probe"), str(probe)], capture_output=True).returncode or \
            subprocess.run([str(d / "probe")], capture_output=True).returncode:
        pytest.skip("the C compiler has no ASAN/UBSAN runtime")
    made = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), f"CC={cc}", "ref-asan"],
                          capture_output=True, text=True)
    if "no reference tree" in made.stdout:
        pytest.skip("no reference tree to compile the program from")
    prog = os.path.join(ROOT, "oracle", "_ref", "ref_forward_asan")
    assert made.returncode == 0 and os.path.exists(prog), made.stdout + made.stderr
    return prog


def run_program(prog, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    return subprocess.run([prog, str(path)], capture_output=True, text=True, env=env)


@pytest.mark.parametrize("table", [8, "collide"])
def test_harness_under_sanitizers(harness_program, tmp_path, table):
    """The harness over the corpus from a file, both programs: nothing is
    loaded into Python under a sanitizer."""
    path = tmp_path / "batch.bin"
    F.dump(str(path), table)
    out = run_program(harness_program, path)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    hist = np.bincount(corpus_reference(table)[1], minlength=X.FWD_STAGES).tolist()
    assert out.stdout.split("stages")[1].split() == [str(h) for h in hist]


def test_harness_program_refuses_malformed_files(harness_program, tmp_path):
    """A file cut short, and one with a frame longer than its slot: refused with
    a message, no sanitizer report."""
    path = tmp_path / "batch.bin"
    F.dump(str(path), 8)
    whole = path.read_bytes()
    short = tmp_path / "short.bin"
    short.write_bytes(whole[:len(whole) // 2])
    long_frame = bytearray(whole)
    long_frame[24:28] = (F.MAXLEN + 1).to_bytes(4, "little")          # lens[0]
    longer = tmp_path / "long.bin"
    longer.write_bytes(bytes(long_frame))
    for bad in (short, longer):
        out = run_program(harness_program, bad)
        assert out.returncode == 2 and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr

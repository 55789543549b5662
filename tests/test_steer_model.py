"""CPU tests that pin tests/steermodel.py, the model the GPU tests of
xfg_steer_egress compare against: the hash against known answers and against
the reference's own header, the queue choice against hand-written rows (one a
branch of the reference's programs), the partition against a per-record walk.
The rows' answers (WANT) were written by hand; test_steer_reference.py
recomputes them from the reference's programs run on the host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import steermodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def le32(b):
    return int.from_bytes(b, "little")


# ---- the hash
def test_hash_known_answers():
    """Computed from the reference's hash_func01.h compiled for the host."""
    s = (le32(bytes([10, 0, 0, 1])) + le32(bytes([10, 0, 0, 2]))) & 0xffffffff
    assert M.superfasthash4(s, M.INITVAL + 17) == 0xf689e196
    assert M.superfasthash4(s, M.INITVAL + 6) == 0x7b5cccf2
    assert M.superfasthash4(0, M.INITVAL + 0) == 0x396d0a7d
    assert M.superfasthash4(0xffffffff, M.INITVAL + 255) == 0x0739c2f1


def reference_tree():
    """Where the build looks for it: $REF, else oracle/Makefile's default."""
    ref = os.environ.get("REF")
    if not ref:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1)
    return ref


def test_hash_against_the_references_header(tmp_path):
    ref = reference_tree()
    if not os.path.isfile(os.path.join(ref, "xdp-bench", "hash_func01.h")):
        pytest.skip("no reference tree")
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    exe = tmp_path / "steer_hash"
    subprocess.run([cc, "-O1", "-w", "-I", os.path.join(ref, "xdp-bench"), "-o", str(exe),
                    os.path.join(HERE, "steer_hash.c")], check=True)
    rng = np.random.default_rng(4096)
    sums = rng.integers(0, 2**32, 4096, dtype=np.uint64)
    protos = rng.integers(0, 256, 4096)
    sums[:4] = [0, 0xffffffff, 0x0000ffff, 0xffff0000]
    text = "".join(f"{int(s):x} {M.INITVAL + int(p):x}\n" for s, p in zip(sums, protos))
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout
    got = [int(line, 16) for line in out.split()]
    assert len(got) == 4096
    want = [M.superfasthash4(int(s), M.INITVAL + int(p)) for s, p in zip(sums, protos)]
    assert got == want


# ---- the queue choice, a row a branch
ROWS = dict(M.hand_rows())
H10 = 0xf689e196        # 10.0.0.1 + 10.0.0.2, UDP (above)
A6, B6 = bytes(range(1, 17)), bytes(range(101, 117))
S6 = sum(le32((A6 + B6)[4 * j:4 * j + 4]) for j in range(8)) & 0xffffffff
# name -> key in (L4_HASH, L4_SPORT, L4_DPORT); None: refused
WANT = {
    "v4_udp": (H10, 4000, 53),
    "v4_udp_tag": (H10, 4000, 53),
    "v4_udp_qinq": (H10, 4000, 53),
    "v4_udp_three_tags": (0, 0, 0),             # a VLAN ethertype is left: default
    "ethertype_05ff": (None, None, None),
    "short_13": (None, None, None),
    "tag_cut_17": (None, None, None),
    "second_tag_cut_21": (None, None, None),
    "v4_cut_l3_19": (0, 0, 0),
    "v4_exact_l3_20": (H10, 0, 0),              # the addresses are there, a UDP header is not
    "v6_qinq_61": (0, 0, 0),
    "v6_qinq_62": (M.superfasthash4(S6, M.INITVAL + 17), 0, 0),
    "v6_udp": (M.superfasthash4(S6, M.INITVAL + 17), 4000, 53),
    "v6_tcp_tag": (M.superfasthash4(S6, M.INITVAL + 6), 40000, 443),
    "v6_tcp_qinq": (M.superfasthash4(S6, M.INITVAL + 6), 40001, 8443),
    "v6_udp_qinq": (M.superfasthash4(S6, M.INITVAL + 17), 40002, 4789),
    "arp": (0, 0, 0),
    "v4_ihl6_udp": (H10, 7, 9),                 # read at l3 + 20, not l3 + 24
    "udp_7_bytes": (H10, 0, 0),
    "udp_8_bytes": (H10, 4000, 53),
    "tcp_19_bytes": (0x7b5cccf2, 0, 0),
    "tcp_20_bytes": (0x7b5cccf2, 4001, 80),
    "icmp": (M.superfasthash4(le32(bytes([10, 0, 0, 1])) + le32(bytes([10, 0, 0, 2])), M.INITVAL + 1),
             0, 0),
    "v4_udp_swapped": (H10, 53, 4000),
    "v6_udp_swapped": (M.superfasthash4(S6, M.INITVAL + 17), 53, 4000),
}


def test_every_row_has_an_answer():
    assert sorted(ROWS) == sorted(WANT)
    assert len(ROWS["short_13"]) == 13 and len(ROWS["tag_cut_17"]) == 17
    assert len(ROWS["v6_qinq_61"]) == 61 and len(ROWS["v6_qinq_62"]) == 62
    assert ROWS["v4_ihl6_udp"][14] == 0x46


@pytest.mark.parametrize("name", sorted(WANT))
def test_hand_written_rows(name):
    f = ROWS[name]
    for mode in (M.L4_HASH, M.L4_SPORT, M.L4_DPORT):
        assert M.key_of(f, mode) == WANT[name][mode], (name, mode)
    # through the avail table: 5 entries over 3 queues, queue 2 for the refused
    avail = [1, 0, 1, 2, 0]
    for mode in (M.L4_HASH, M.L4_SPORT, M.L4_DPORT):
        k = WANT[name][mode]
        want = (2, True) if k is None else (avail[k % 5], False)
        assert M.queue_of_frame(f, mode, avail, 2) == want


def test_symmetric_hashing():
    for a, b in (("v4_udp", "v4_udp_swapped"), ("v6_udp", "v6_udp_swapped")):
        for nq in (2, 7, 64):
            av = list(range(nq))
            assert M.queue_of_frame(ROWS[a], M.L4_HASH, av, 0) == M.queue_of_frame(ROWS[b], M.L4_HASH, av, 0)


def test_refused_frames_take_skip_queue_and_are_counted():
    names = ["short_13", "v4_udp", "tag_cut_17", "ethertype_05ff", "second_tag_cut_21"]
    frames = [ROWS[n] for n in names]
    addr = np.arange(5, dtype=np.uint64) * np.uint64(2048)
    lens = np.array([len(f) for f in frames], np.uint32)
    v = np.array([2, 2, 2, 1, 2], np.uint8)          # the 0x05ff frame is not PASS: not parsed
    tx, fill, counts, qof = M.steer_model(frames, addr, lens, v, 4, M.L4_HASH, skip_queue=3)
    q = H10 % 4
    assert qof.tolist() == [3, q, 3, M.QUEUE_NONE, 3]
    want = [0, 0, 0, 3, 1, 3]
    want[q] += 1
    assert counts.tolist() == want
    assert tx[3][:, 0].tolist() == [0, 2 * 2048, 4 * 2048] and tx[3][:, 1].tolist() == [13, 17, 21]
    assert fill.tolist() == [3 * 2048]


# ---- the partition
def test_model_against_the_walk():
    rng = np.random.default_rng(5)
    rows = [f for _, f in M.hand_rows()]
    for nq, avail in ((1, None), (2, None), (3, [2, 2, 0, 1]), (7, None), (64, None),
                      (5, list(rng.integers(0, 5, 256)))):
        for p in (0.0, 0.6, 1.0):
            n = 300
            frames = []
            for i in range(n):
                if i % 4 == 0:
                    frames.append(rows[int(rng.integers(len(rows)))])
                else:
                    a, b = bytes(rng.integers(0, 256, 4, dtype=np.uint8)), bytes(rng.integers(0, 256, 4, dtype=np.uint8))
                    frames.append(M.eth(M.ETH_P_IP, M.ipv4(a, b, 17, M.udp(int(rng.integers(65536)),
                                                                              int(rng.integers(65536))))))
            addr = rng.integers(0, 2**63, n, dtype=np.uint64)
            lens = np.array([len(f) for f in frames], np.uint32)
            v = np.where(rng.random(n) < p, 2, rng.integers(0, 256, n)).astype(np.uint8)
            for mode in (M.L4_HASH, M.L4_SPORT, M.L4_DPORT):
                tx, fill, counts, qof = M.steer_model(frames, addr, lens, v, nq, mode, avail, nq - 1)
                w = M.walk(frames, addr, lens, v, nq, mode, avail, nq - 1)
                assert [t.tolist() for t in tx] == [[list(r) for r in t] for t in w[0]]
                assert fill.tolist() == w[1] and counts.tolist() == w[2] and qof.tolist() == w[3]
                assert counts.dtype == np.uint64
                assert int(counts[:nq + 1].sum()) == n

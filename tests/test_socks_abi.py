"""CPU tests of xfg_classify_socks and xfg_socks_egress (include/xdpfilter_gpu.h):
the symbols in both libraries, the structures' layout against the header, the
argument checks on a host-only context (device pointers are made-up numbers: no
one is dereferenced before the context is found to have no device; the socket
table is host memory and is read), and the numpy model of the GPU tests against
hand-written rows and a plain walk."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import xfgpu as G
from sockmodel import sock_model, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
EINVAL, ENODEV = -errno.EINVAL, -errno.ENODEV


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbols_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    for sym in ("xfg_classify_socks", "xfg_socks_egress"):
        assert hasattr(lib, sym)
        assert sym in G.EXPORTS


FIELDS = {
    "xfg_sock": (G.Sock, ["rx_descs", "rx_first", "rx_mask", "tx_descs", "tx_first", "tx_mask",
                          "fill_addrs", "fill_first", "fill_mask", "count"]),
    "xfg_socks": (G.Socks, ["sz", "umem", "socks", "flat", "nsocks"]),
    "xfg_socks_egress": (G.SocksEgress, ["sz", "fill_addrs", "fill_first", "fill_mask", "counts",
                                         "flags"]),
}


def test_structures_and_constants_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    body = ""
    for st, (_, fields) in FIELDS.items():
        body += f'printf("{st}.sizeof %zu\\n", sizeof(struct {st}));\n'
        for f in fields:
            body += f'printf("{st}.{f} %zu\\n", offsetof(struct {st}, {f}));\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\n' + body +
                   'printf("max %u\\n", XFG_SOCKS_MAX);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for st, (cls, fields) in FIELDS.items():
        assert int(out[st + ".sizeof"]) == C.sizeof(cls), st
        assert [n for n, _ in cls._fields_] == fields
        for f in fields:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, (st, f)
    assert int(out["max"]) == G.SOCKS_MAX == 1024
    # the two top-level structures start with their size, as xfg_egress does
    assert G.Socks.sz.offset == G.SocksEgress.sz.offset == 0


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


def sock(**kw):
    f = dict(rx_descs=0x20000, rx_first=0, rx_mask=0xffffffff, tx_descs=0x30000, tx_first=0,
             tx_mask=0xffffffff, fill_addrs=0x40000, fill_first=0, fill_mask=0xffffffff, count=64)
    f.update(kw)
    return f


def socks(table, **kw):
    tab = G.sock_table(table)
    f = dict(sz=C.sizeof(G.Socks), umem=0x10000, socks=tab, flat=None, nsocks=len(table))
    f.update(kw)
    sk = G.Socks(f["sz"], f["umem"], f["socks"], f["flat"], f["nsocks"])
    sk._keep = tab
    return sk


def egress(**kw):
    f = dict(sz=C.sizeof(G.SocksEgress), fill_addrs=None, fill_first=0, fill_mask=0xffffffff,
             counts=0x50000, flags=0)
    f.update(kw)
    return G.SocksEgress(f["sz"], f["fill_addrs"], f["fill_first"], f["fill_mask"], f["counts"],
                         f["flags"])


def classify(ctx, sk, verdicts=0x60000):
    return G.lib.xfg_classify_socks(ctx, 0, None if sk is None else C.byref(sk), verdicts, None)


def egr(ctx, sk, e, verdicts=0x60000):
    return G.lib.xfg_socks_egress(ctx, 0, None if sk is None else C.byref(sk),
                                  None if e is None else C.byref(e), verdicts, None)


GOOD = [
    [sock()],
    [sock(count=0), sock(count=5), sock(count=0), sock(count=0), sock(), sock(count=0)],
    [sock(rx_mask=63, tx_mask=63, fill_mask=63, rx_first=0xfffffff0)] * 64,
    [sock(count=0, rx_descs=None, tx_descs=None, fill_addrs=None)],          # nothing peeked
    [sock(count=3)] * 1024,
    [sock(count=2**32 - 2), sock(count=1)],                                  # total 2^32 - 1
]


@pytest.mark.parametrize("table", range(len(GOOD)))
def test_host_only_context_is_enodev(host_only, table):
    ctx = host_only.ctx
    sk = socks(GOOD[table])
    assert classify(ctx, sk) == ENODEV
    assert classify(ctx, socks(GOOD[table], flat=0x70000)) == ENODEV
    assert classify(ctx, socks(GOOD[table], sz=C.sizeof(G.Socks) + 8)) == ENODEV
    assert egr(ctx, sk, egress()) == ENODEV
    assert egr(ctx, sk, egress(fill_addrs=0x80000)) == ENODEV
    assert egr(ctx, sk, egress(flags=G.EGRESS_SWAP_MACS)) == ENODEV
    assert egr(ctx, sk, egress(sz=C.sizeof(G.SocksEgress) + 8)) == ENODEV


def test_host_only_binding_raises(host_only):
    for call in (lambda: host_only.classify_socks(0x10000, [sock()], 0x60000),
                 lambda: host_only.socks_egress([sock()], 0x60000, 0x50000)):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    # an empty round is still a call on a context without a device
    assert classify(host_only.ctx, socks([sock(count=0)]), verdicts=None) == ENODEV
    assert classify(host_only.ctx, socks([sock(count=0)], umem=None), verdicts=None) == ENODEV


BAD_SOCKS = [
    dict(sz=C.sizeof(G.Socks) - 1), dict(sz=0), dict(socks=None), dict(nsocks=0),
    dict(nsocks=1025),
]
BAD_TABLES = [
    [sock(), sock(rx_descs=None)],                       # records but no ring
    [sock(rx_descs=0x20004)],                            # not 8-byte aligned
    [sock(rx_mask=62)], [sock(rx_mask=0x7ffffffe)],      # not 2^k - 1
    [sock(count=0, rx_mask=5)],                          # ... in an empty socket too
    [sock(rx_mask=31)],                                  # 64 records from a ring of 32
    [sock(count=0), sock(rx_mask=63, count=65)],
    [sock(count=2**32 - 1), sock(count=1)],              # total 2^32
    [sock(count=2**31)] * 2,
]


def test_einval_both_calls(host_only):
    ctx = host_only.ctx
    good = socks([sock()] * 3)
    assert classify(None, good) == EINVAL and egr(None, good, egress()) == EINVAL
    assert classify(ctx, None) == EINVAL and egr(ctx, None, egress()) == EINVAL
    for kw in BAD_SOCKS:
        many = [sock()] * 1025 if kw.get("nsocks") == 1025 else [sock()] * 3
        sk = socks(many, **kw)
        assert classify(ctx, sk) == EINVAL, kw
        assert egr(ctx, sk, egress()) == EINVAL, kw
    for table in BAD_TABLES:
        sk = socks(table)
        assert classify(ctx, sk) == EINVAL, table
        assert egr(ctx, sk, egress()) == EINVAL, table


def test_einval_classify(host_only):
    ctx = host_only.ctx
    assert classify(ctx, socks([sock()], umem=None)) == EINVAL
    assert classify(ctx, socks([sock()]), verdicts=None) == EINVAL
    assert classify(ctx, socks([sock()], flat=0x70008)) == EINVAL
    assert classify(ctx, socks([sock()], flat=0x70001)) == EINVAL
    assert classify(ctx, socks([sock(count=0)], flat=0x70008), verdicts=None) == EINVAL


def test_einval_egress(host_only):
    ctx = host_only.ctx
    sk = socks([sock(count=0), sock(), sock(count=7)])
    assert egr(ctx, sk, None) == EINVAL
    assert egr(ctx, sk, egress(sz=C.sizeof(G.SocksEgress) - 1)) == EINVAL
    assert egr(ctx, sk, egress(counts=None)) == EINVAL
    assert egr(ctx, sk, egress(counts=0x50004)) == EINVAL
    assert egr(ctx, sk, egress(flags=G.EGRESS_MULTIBUF)) == EINVAL
    assert egr(ctx, sk, egress(flags=G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS)) == EINVAL
    assert egr(ctx, sk, egress(flags=2)) == EINVAL
    assert egr(ctx, sk, egress(flags=1 << 31)) == EINVAL
    assert egr(ctx, socks([sock()], umem=None), egress(flags=G.EGRESS_SWAP_MACS)) == EINVAL
    assert egr(ctx, socks([sock()], umem=None), egress()) == ENODEV      # (needed for the swap only)
    assert egr(ctx, sk, egress(), verdicts=None) == EINVAL               # a TX ring and records
    no_tx = socks([sock(tx_descs=None), sock(count=0)])
    assert egr(ctx, no_tx, egress(), verdicts=None) == ENODEV            # rx_drop reads none
    # the shared fill ring: total entries
    assert egr(ctx, sk, egress(fill_addrs=0x80000, fill_mask=63)) == EINVAL    # 71 records
    assert egr(ctx, sk, egress(fill_addrs=0x80000, fill_mask=127)) == ENODEV
    assert egr(ctx, sk, egress(fill_addrs=0x80000, fill_mask=126)) == EINVAL
    assert egr(ctx, sk, egress(fill_addrs=0x80004)) == EINVAL
    # every ring that is written: its socket's count
    for bad in (dict(tx_mask=31), dict(tx_mask=62), dict(tx_descs=0x30004), dict(fill_mask=31),
                dict(fill_mask=62), dict(fill_addrs=0x40004)):
        assert egr(ctx, socks([sock(count=0), sock(**bad)]), egress()) == EINVAL, bad
    # ... and a socket's own fill fields are ignored beside the shared ring
    for ignored in (dict(fill_mask=31), dict(fill_mask=62), dict(fill_addrs=0x40004)):
        assert egr(ctx, socks([sock(**ignored)]), egress(fill_addrs=0x80000)) == ENODEV, ignored


def test_a_refused_call_writes_nothing(host_only):
    ctx = host_only.ctx
    for table, ekw in (([sock(), sock(rx_mask=62)], {}), ([sock()] * 3, dict(flags=2)),
                       ([sock()] * 2, dict(fill_addrs=0x80000, fill_mask=63))):
        sk, e = socks(table), egress(**ekw)
        before = (bytes(sk._keep), bytes(sk), bytes(e))
        assert classify(ctx, sk) in (EINVAL, ENODEV)
        assert egr(ctx, sk, e) == EINVAL
        assert (bytes(sk._keep), bytes(sk), bytes(e)) == before


# ---- the model
A = 1 << 48         # an offset in bits 48..63 stays in a TX record, not in a fill address
ROWS = [
    # counts, verdicts, has_tx, has_fill -> TX addrs a socket, own fill a socket, shared fill, counts
    ([3], [2, 1, 2], None, None, [[0, 2]], [[1]], [1], [2, 1, 2, 1]),
    ([0, 2], [2, 2], None, None, [[], [0, 1]], [[], []], [], [0, 0, 2, 0, 2, 0]),            # empty first
    ([2, 0, 1], [1, 2, 2], None, None, [[1], [], [2]], [[0], [], []], [0],
     [1, 1, 0, 0, 1, 0, 2, 1]),                                                             # in the middle
    ([2, 0], [0, 3], None, None, [[], []], [[0, 1], []], [0, 1], [0, 2, 0, 0, 0, 2]),         # last
    ([1, 0, 0, 2], [2, 1, 2], None, None, [[0], [], [], [2]], [[], [], [], [1]], [1],
     [1, 0, 0, 0, 0, 0, 1, 1, 2, 1]),                                                       # two adjacent
    ([0, 0], [], None, None, [[], []], [[], []], [], [0] * 6),
    ([2, 2], [2, 2, 2, 1], [False, True], None, [[], [2]], [[0, 1], [3]], [0, 1, 3],
     [0, 2, 1, 1, 1, 3]),                                                                   # no TX ring: rx_drop
    ([2, 2], [1, 2, 1, 255], None, [False, True], [[1], []], [[], [2, 3]], [0, 2, 3],
     [1, 1, 0, 2, 1, 3]),                                                                   # no fill ring
]


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_model_against_hand_written_rows(row):
    counts, v, has_tx, has_fill, want_tx, want_own, want_shared, want_counts = ROWS[row]
    n = sum(counts)
    addr = (np.arange(n, dtype=np.uint64) * np.uint64(4096)) | np.uint64(A)
    lens = np.arange(n, dtype=np.uint32) + 60
    v = np.array(v, np.uint8)
    for shared in (False, True):
        tx, fill, out = sock_model(counts, addr, lens, v, has_tx, has_fill, shared)
        assert out.tolist() == want_counts and out.dtype == np.uint64
        for s, idx in enumerate(want_tx):
            assert tx[s].tolist() == [[int(addr[i]), int(lens[i])] for i in idx]
        if shared:
            assert fill.tolist() == [i * 4096 for i in want_shared]
        else:
            assert [f.tolist() for f in fill] == [[i * 4096 for i in own] for own in want_own]
        w = walk(counts, addr, lens, v, has_tx, has_fill, shared)
        assert w[0] == [t.tolist() for t in tx] and w[2] == out.tolist()
        assert w[1] == (fill.tolist() if shared else [f.tolist() for f in fill])


def test_model_against_the_walk_on_random_inputs():
    rng = np.random.default_rng(11)
    for S in (1, 2, 7, 64, 300):
        for p in (0.0, 0.5, 1.0):
            counts = rng.integers(0, 5, S) * (rng.random(S) < 0.7)
            n = int(counts.sum())
            addr = rng.integers(0, 2**63, n, dtype=np.uint64)
            lens = rng.integers(14, 1515, n).astype(np.uint32)
            v = np.where(rng.random(n) < p, 2, rng.integers(0, 256, n)).astype(np.uint8)
            has_tx, has_fill = rng.random(S) < 0.8, rng.random(S) < 0.8
            for shared in (False, True):
                tx, fill, out = sock_model(counts, addr, lens, v, has_tx, has_fill, shared)
                w = walk(counts, addr, lens, v, has_tx, has_fill, shared)
                assert w[0] == [t.tolist() for t in tx] and w[2] == out.tolist()
                assert w[1] == (fill.tolist() if shared else [f.tolist() for f in fill])
                assert int(out[2 * S]) + int(out[2 * S + 1]) == n

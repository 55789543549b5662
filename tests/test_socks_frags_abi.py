"""CPU tests of xfg_classify_socks_frags and xfg_socks_frags_egress
(include/xdpfilter_gpu.h): the symbols in both libraries, the structure's layout
and the two constants against the header, the argument checks on a host-only
context (device pointers are made-up numbers: no one is dereferenced before the
context is found to have no device; the socket table and done[] are host memory
and are read), and the numpy model of the GPU tests against hand-written rows
and a plain walk."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import xfgpu as G
from sockfragmodel import PKT_NONE, VERDICT_NONE, classify_model, egress_model, spread, swapped, walk
from test_socks_abi import BAD_SOCKS, BAD_TABLES, GOOD, egress, sock, socks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
EINVAL, ENODEV = -errno.EINVAL, -errno.ENODEV


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbols_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    for sym in ("xfg_classify_socks_frags", "xfg_socks_frags_egress"):
        assert hasattr(lib, sym)
        assert sym in G.EXPORTS


def test_structure_and_constants_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    fields = ["sz", "done", "pkt_of", "counts"]
    body = 'printf("sizeof %zu\\n", sizeof(struct xfg_socks_frags));\n'
    for f in fields:
        body += f'printf("{f} %zu\\n", offsetof(struct xfg_socks_frags, {f}));\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\n' + body +
                   'printf("vnone %u\\n", XFG_VERDICT_NONE);\n'
                   'printf("pnone %u\\n", XFG_PKT_NONE);\n'
                   'printf("socks %zu\\n", sizeof(struct xfg_socks));\n'
                   'printf("egress %zu\\n", sizeof(struct xfg_socks_egress));\n'
                   'printf("sock %zu\\n", sizeof(struct xfg_sock));\n'
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(G.SocksFrags)
    assert [n for n, _ in G.SocksFrags._fields_] == fields
    for f in fields:
        assert int(out[f]) == getattr(G.SocksFrags, f).offset, f
    assert G.SocksFrags.sz.offset == 0
    assert int(out["vnone"]) == G.VERDICT_NONE == VERDICT_NONE == 0xff
    assert int(out["pnone"]) == G.PKT_NONE == PKT_NONE == 0xffffffff
    assert G.VERDICT_NONE >= 32                  # below no action mask's bit
    # the existing structures keep their sizes
    assert (int(out["socks"]), int(out["egress"]), int(out["sock"])) == \
        (C.sizeof(G.Socks), C.sizeof(G.SocksEgress), C.sizeof(G.Sock)) == (40, 40, 56)


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


def frags(nsocks=1024, **kw):
    done = (C.c_uint32 * nsocks)(*([0xA5A5A5A5] * nsocks))
    f = dict(sz=C.sizeof(G.SocksFrags), done=done, pkt_of=0x90000)
    f.update(kw)
    fr = G.SocksFrags(f["sz"], f["done"], f["pkt_of"])
    for k in range(3):
        fr.counts[k] = 0xA5
    fr._keep = done
    return fr


def classify(ctx, sk, fr, verdicts=0x60000):
    return G.lib.xfg_classify_socks_frags(ctx, 0, None if sk is None else C.byref(sk),
                                          None if fr is None else C.byref(fr), verdicts, None)


def egr(ctx, sk, e, done=None, verdicts=0x60000):
    d = None if done is None else (C.c_uint32 * len(done))(*done)
    return G.lib.xfg_socks_frags_egress(ctx, 0, None if sk is None else C.byref(sk),
                                        None if e is None else C.byref(e), d, verdicts, None)


def untouched(fr):
    return list(fr.counts) == [0xA5] * 3 and set(fr._keep) == {0xA5A5A5A5}


@pytest.mark.parametrize("table", range(len(GOOD)))
def test_host_only_context_is_enodev(host_only, table):
    ctx = host_only.ctx
    sk = socks(GOOD[table])
    done = [min(s["count"], 3) for s in GOOD[table]]
    for fr in (frags(), frags(pkt_of=None), frags(sz=C.sizeof(G.SocksFrags) + 8)):
        assert classify(ctx, sk, fr) == ENODEV
        assert untouched(fr)
    assert classify(ctx, socks(GOOD[table], flat=0x70000), frags()) == ENODEV
    for flags in (0, G.EGRESS_SWAP_MACS, G.EGRESS_MULTIBUF, G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS):
        assert egr(ctx, sk, egress(flags=flags)) == ENODEV
        assert egr(ctx, sk, egress(flags=flags), done=done) == ENODEV
    assert egr(ctx, sk, egress(fill_addrs=0x80000), done=[0] * len(done)) == ENODEV
    assert egr(ctx, sk, egress(), done=[s["count"] for s in GOOD[table]]) == ENODEV


def test_host_only_binding_raises(host_only):
    for call in (lambda: host_only.classify_socks_frags(0x10000, [sock()], 0x60000),
                 lambda: host_only.socks_frags_egress([sock()], 0x60000, 0x50000, done=[64]),
                 lambda: host_only.socks_frags_egress([sock()], 0x60000, 0x50000)):
        with pytest.raises(OSError) as e:
            call()
        assert e.value.errno == errno.ENODEV
    # an empty round is still a call on a context without a device
    assert classify(host_only.ctx, socks([sock(count=0)]), frags(), verdicts=None) == ENODEV
    assert classify(host_only.ctx, socks([sock(count=0)], umem=None), frags(), verdicts=None) == ENODEV


def test_einval_what_the_single_buffer_calls_refuse(host_only):
    ctx = host_only.ctx
    good = socks([sock()] * 3)
    assert classify(None, good, frags()) == EINVAL and egr(None, good, egress()) == EINVAL
    assert classify(ctx, None, frags()) == EINVAL and egr(ctx, None, egress()) == EINVAL
    for kw in BAD_SOCKS:
        many = [sock()] * 1025 if kw.get("nsocks") == 1025 else [sock()] * 3
        sk = socks(many, **kw)
        assert classify(ctx, sk, frags(nsocks=1025)) == EINVAL, kw
        assert egr(ctx, sk, egress()) == EINVAL, kw
    for table in BAD_TABLES:
        sk = socks(table)
        fr = frags()
        assert classify(ctx, sk, fr) == EINVAL, table
        assert untouched(fr)
        assert egr(ctx, sk, egress()) == EINVAL, table
    # xfg_classify_socks' own
    assert classify(ctx, socks([sock()], umem=None), frags()) == EINVAL
    assert classify(ctx, socks([sock()]), frags(), verdicts=None) == EINVAL
    assert classify(ctx, socks([sock()], flat=0x70008), frags()) == EINVAL
    assert classify(ctx, socks([sock(count=0)], flat=0x70001), frags(), verdicts=None) == EINVAL


def test_einval_classify(host_only):
    ctx = host_only.ctx
    sk = socks([sock(count=0), sock(), sock(count=7)])
    assert classify(ctx, sk, None) == EINVAL
    assert classify(ctx, sk, frags(sz=C.sizeof(G.SocksFrags) - 1)) == EINVAL
    assert classify(ctx, sk, frags(sz=0)) == EINVAL
    assert classify(ctx, sk, frags(done=None)) == EINVAL
    for bad in (0x90001, 0x90002, 0x90003):
        fr = frags(pkt_of=bad)
        assert classify(ctx, sk, fr) == EINVAL
        assert untouched(fr)                      # a refused call writes nothing
    assert classify(ctx, sk, frags(pkt_of=0x90004)) == ENODEV


def test_einval_egress(host_only):
    ctx = host_only.ctx
    sk = socks([sock(count=0), sock(), sock(count=7)])
    assert egr(ctx, sk, None) == EINVAL
    assert egr(ctx, sk, egress(sz=C.sizeof(G.SocksEgress) - 1)) == EINVAL
    assert egr(ctx, sk, egress(counts=None)) == EINVAL
    assert egr(ctx, sk, egress(counts=0x50004)) == EINVAL
    for flags in (2, 8, 1 << 31, G.EGRESS_MULTIBUF | 2, G.EGRESS_SWAP_MACS | 8):
        assert egr(ctx, sk, egress(flags=flags)) == EINVAL, flags
    for flags in (G.EGRESS_SWAP_MACS, G.EGRESS_SWAP_MACS | G.EGRESS_MULTIBUF):
        assert egr(ctx, socks([sock()], umem=None), egress(flags=flags)) == EINVAL
    assert egr(ctx, socks([sock()], umem=None), egress(flags=G.EGRESS_MULTIBUF)) == ENODEV
    assert egr(ctx, sk, egress(), verdicts=None) == EINVAL               # a TX ring and records
    no_tx = socks([sock(tx_descs=None), sock(count=0)])
    assert egr(ctx, no_tx, egress(), verdicts=None) == ENODEV            # rx_drop reads none
    # done[s] above the socket's count
    assert egr(ctx, sk, egress(), done=[0, 64, 7]) == ENODEV
    assert egr(ctx, sk, egress(), done=[0, 0, 0]) == ENODEV
    for done in ([1, 64, 7], [0, 65, 7], [0, 64, 8], [0, 2**32 - 1, 0]):
        assert egr(ctx, sk, egress(), done=done) == EINVAL, done
    # ring sizes against count, not done: the shared fill ring needs total entries
    assert egr(ctx, sk, egress(fill_addrs=0x80000, fill_mask=63), done=[0, 1, 1]) == EINVAL   # 71 records
    assert egr(ctx, sk, egress(fill_addrs=0x80000, fill_mask=127), done=[0, 1, 1]) == ENODEV
    assert egr(ctx, sk, egress(fill_addrs=0x80004)) == EINVAL
    for bad in (dict(tx_mask=31), dict(tx_mask=62), dict(tx_descs=0x30004), dict(fill_mask=31),
                dict(fill_mask=62), dict(fill_addrs=0x40004)):
        assert egr(ctx, socks([sock(count=0), sock(**bad)]), egress(), done=[0, 1]) == EINVAL, bad
    for ignored in (dict(fill_mask=31), dict(fill_mask=62), dict(fill_addrs=0x40004)):
        assert egr(ctx, socks([sock(**ignored)]), egress(fill_addrs=0x80000)) == ENODEV, ignored


def test_the_single_buffer_egress_still_refuses_multibuf(host_only):
    from test_socks_abi import egr as plain
    sk = socks([sock()])
    assert plain(host_only.ctx, sk, egress(flags=G.EGRESS_MULTIBUF)) == EINVAL
    assert plain(host_only.ctx, sk, egress(flags=G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS)) == EINVAL


# ---- the model
K, E = 1, 0          # continued, end of packet
N = PKT_NONE
ROWS = [
    # counts, options, packet verdicts -> done, pkt_of, heads, counts,
    #   TX record indices a socket, own fill a socket, shared fill, egress counts, swapped
    # a socket with no end-of-packet record between two that have one
    ([3, 2, 2], [K, E, K, K, K, E, E], [2, 1, 2],
     [2, 0, 2], [0, 0, N, N, N, 1, 2], [1, 0, 0, 0, 0, 1, 1], (3, 4, 3),
     [[0, 1], [], [6]], [[], [], [5]], [5], [2, 0, 0, 0, 1, 1, 3, 1], [0, 6]),
    # empty sockets: first, in the middle (a run), last
    ([0, 2, 0, 0, 1, 0], [E, E, E], [1, 2, 2],
     [0, 2, 0, 0, 1, 0], [0, 1, 2], [1, 1, 1], (3, 3, 0),
     [[], [1], [], [], [2], []], [[], [0], [], [], [], []], [0],
     [0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 2, 1], [1, 2]),
    # a socket that is one whole packet, PASS and not
    ([4, 3], [K, K, K, E, K, K, E], [2, 0],
     [4, 3], [0, 0, 0, 0, 1, 1, 1], [1, 0, 0, 0, 1, 0, 0], (2, 7, 0),
     [[0, 1, 2, 3], []], [[], [4, 5, 6]], [4, 5, 6], [4, 0, 0, 3, 4, 3], [0]),
    # record 0 of a socket starts a packet whatever the socket before ended with
    ([2, 2], [E, K, K, E], [1, 2],
     [1, 2], [0, N, 1, 1], [1, 0, 1, 0], (2, 3, 1),
     [[], [2, 3]], [[0], []], [0], [0, 1, 2, 0, 2, 1], [2]),
    # no end-of-packet record at all
    ([2, 1], [K, K, K], [],
     [0, 0], [N, N, N], [0, 0, 0], (0, 0, 3),
     [[], []], [[], []], [], [0, 0, 0, 0, 0, 0], []),
    ([0, 0], [], [], [0, 0], [], [], (0, 0, 0), [[], []], [[], []], [], [0] * 6, []),
]
A = 1 << 48          # an offset in bits 48..63 stays in a TX record, not in a fill address


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_model_against_hand_written_rows(row):
    (counts, opts, pv, w_done, w_pkt, w_heads, w_counts, w_tx, w_own, w_shared, w_out,
     w_swap) = ROWS[row]
    n = sum(counts)
    opts = np.array(opts, np.uint32) | np.uint32(1 << 16)        # other option bits are ignored
    addr = (np.arange(n, dtype=np.uint64) * np.uint64(4096)) | np.uint64(A)
    lens = np.arange(n, dtype=np.uint32) + 60
    done, pkt_of, heads, c3 = classify_model(counts, opts)
    assert done.tolist() == w_done and done.dtype == np.uint32
    assert pkt_of.tolist() == w_pkt and pkt_of.dtype == np.uint32
    assert heads.astype(int).tolist() == w_heads and c3 == w_counts
    assert int(heads.sum()) == c3[0] == len(pv) and c3[1] + c3[2] == n
    v = spread(pkt_of, pv)
    assert v.tolist() == [VERDICT_NONE if p == N else pv[p] for p in w_pkt]

    def rec(i):
        return [int(addr[i]), int(lens[i]) | ((int(opts[i]) & 1) << 32)]

    for shared in (False, True):
        tx, fill, out = egress_model(counts, done, addr, lens, opts, v, shared=shared)
        assert out.tolist() == w_out
        assert [t.tolist() for t in tx] == [[rec(i) for i in idx] for idx in w_tx]
        if shared:
            assert fill.tolist() == [i * 4096 for i in w_shared]
        else:
            assert [f.tolist() for f in fill] == [[i * 4096 for i in own] for own in w_own]
        w = walk(counts, addr, lens, opts, pv, shared=shared)
        assert w[0] == w_done and w[1] == w_pkt and w[2] == v.tolist()
        assert [int(h) for h in w[3]] == w_heads and w[4] == w_counts
        assert w[5] == [t.tolist() for t in tx] and w[7] == w_out
        assert w[6] == (fill.tolist() if shared else [f.tolist() for f in fill])
        assert np.flatnonzero(w[8]).tolist() == w_swap
        assert np.flatnonzero(swapped(counts, done, opts, v)).tolist() == w_swap


def test_model_against_the_walk_on_random_inputs():
    rng = np.random.default_rng(13)
    for S in (1, 2, 7, 64, 300):
        for p in (0.0, 0.4, 0.9, 1.0):
            counts = rng.integers(0, 6, S) * (rng.random(S) < 0.7)
            n = int(counts.sum())
            opts = (rng.random(n) < p).astype(np.uint32) | (rng.integers(0, 4, n).astype(np.uint32) << 1)
            addr = rng.integers(0, 2**63, n, dtype=np.uint64)
            lens = rng.integers(14, 1515, n).astype(np.uint32)
            has_tx, has_fill = rng.random(S) < 0.8, rng.random(S) < 0.8
            done, pkt_of, heads, c3 = classify_model(counts, opts)
            pv = np.where(rng.random(c3[0]) < 0.5, 2, rng.integers(0, 5, c3[0])).astype(np.uint8)
            v = spread(pkt_of, pv)
            assert np.all(done <= counts) and c3[1] == int(done.sum())
            for shared in (False, True):
                tx, fill, out = egress_model(counts, done, addr, lens, opts, v, has_tx, has_fill, shared)
                w = walk(counts, addr, lens, opts, pv, has_tx, has_fill, shared)
                assert w[0] == done.tolist() and w[1] == pkt_of.tolist() and w[2] == v.tolist()
                assert w[3] == heads.tolist() and w[4] == c3
                assert w[5] == [t.tolist() for t in tx] and w[7] == out.tolist()
                assert w[6] == (fill.tolist() if shared else [f.tolist() for f in fill])
                assert w[8] == swapped(counts, done, opts, v, has_tx).tolist()
                assert int(out[2 * S]) + int(out[2 * S + 1]) == c3[1]
            # done == NULL: every record is live, the trailing ones on the fill side
            tx, fill, out = egress_model(counts, None, addr, lens, opts, v, has_tx, has_fill, True)
            assert int(out[2 * S]) + int(out[2 * S + 1]) == n and len(fill) == int(out[2 * S + 1])

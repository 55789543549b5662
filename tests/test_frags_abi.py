"""CPU tests of xfg_classify_descs_frags (include/xdpfilter_gpu.h): the symbol
in both libraries, the structure's layout against the header, the argument
checks on a host-only context (no pointer is dereferenced before the context is
found to have no device), and the numpy model of the GPU tests against
hand-written rows."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import xfgpu as G
from fragmodel import frag_model, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbol_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, "xfg_classify_descs_frags")
    assert "xfg_classify_descs_frags" in G.EXPORTS


def test_structure_and_constants_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\n'
                   'printf("sizeof %zu\\n", sizeof(struct xfg_frags));\n'
                   'printf("sz %zu\\n", offsetof(struct xfg_frags, sz));\n'
                   'printf("pkt_of %zu\\n", offsetof(struct xfg_frags, pkt_of));\n'
                   'printf("counts %zu\\n", offsetof(struct xfg_frags, counts));\n'
                   'printf("contd %u\\n", XFG_XDP_PKT_CONTD);\n'
                   'printf("multibuf %u\\n", XFG_EGRESS_MULTIBUF);\n'
                   'printf("swap %u\\n", XFG_EGRESS_SWAP_MACS);\n'
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(G.Frags)
    assert [name for name, _ in G.Frags._fields_] == ["sz", "pkt_of", "counts"]
    for f in ("sz", "pkt_of", "counts"):
        assert int(out[f]) == getattr(G.Frags, f).offset, f
    assert int(out["contd"]) == G.XDP_PKT_CONTD == 1
    assert int(out["multibuf"]) == G.EGRESS_MULTIBUF
    assert G.EGRESS_MULTIBUF & (G.EGRESS_MULTIBUF - 1) == 0          # one bit, not the swap's
    assert int(out["swap"]) == G.EGRESS_SWAP_MACS != G.EGRESS_MULTIBUF


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


def frags(**kw):
    f = dict(sz=C.sizeof(G.Frags), pkt_of=0x70000)
    f.update(kw)
    fr = G.Frags(f["sz"], f["pkt_of"])
    for k in range(3):
        fr.counts[k] = 0xA5
    return fr


def call(ctx, db, fr, verdicts=0x60000):
    return G.lib.xfg_classify_descs_frags(ctx, 0, None if db is None else C.byref(db),
                                          None if fr is None else C.byref(fr), verdicts, None)


def batch(count=1000, descs=0x20000, mask=0xffffffff):
    return G.DescBatch(0x10000, descs, 0, mask, count)


def test_host_only_context_is_enodev(host_only):
    f = host_only
    assert call(f.ctx, batch(), frags()) == -errno.ENODEV
    assert call(f.ctx, batch(), frags(pkt_of=None)) == -errno.ENODEV
    assert call(f.ctx, batch(count=0), frags(), verdicts=None) == -errno.ENODEV
    assert call(f.ctx, batch(count=2**32 - 1), frags()) == -errno.ENODEV
    assert call(f.ctx, batch(), frags(sz=C.sizeof(G.Frags) + 8)) == -errno.ENODEV
    with pytest.raises(OSError) as e:
        f.classify_descs_frags(0x10000, 0x20000, 16, 0x60000)
    assert e.value.errno == errno.ENODEV
    # the egress flag: a known bit, alone and beside the swap
    from test_egress_abi import call as egress, good
    assert egress(f.ctx, good(flags=G.EGRESS_MULTIBUF)) == -errno.ENODEV
    assert egress(f.ctx, good(flags=G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS)) == -errno.ENODEV
    assert egress(f.ctx, good(flags=G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS, umem=None)) == -errno.EINVAL


def test_einval(host_only):
    ctx = host_only.ctx
    assert call(None, batch(), frags()) == -errno.EINVAL
    assert call(ctx, None, frags()) == -errno.EINVAL
    assert call(ctx, batch(), None) == -errno.EINVAL
    assert call(ctx, batch(), frags(), verdicts=None) == -errno.EINVAL     # as xfg_classify_descs
    assert call(ctx, batch(), frags(sz=C.sizeof(G.Frags) - 1)) == -errno.EINVAL
    assert call(ctx, batch(), frags(sz=0)) == -errno.EINVAL
    assert call(ctx, batch(), frags(pkt_of=0x70002)) == -errno.EINVAL
    assert call(ctx, batch(), frags(pkt_of=0x70001)) == -errno.EINVAL
    assert call(ctx, batch(count=2**32), frags()) == -errno.EINVAL
    fr = frags(pkt_of=0x70002)
    assert call(ctx, batch(), fr) == -errno.EINVAL
    assert list(fr.counts) == [0xA5] * 3            # a refused call writes nothing


K, E = 1, 0          # continued, end of packet (other option bits are ignored)
ROWS = [
    # options, pkt_of, heads, (packets, frags_done, trailing)
    ([E, E, E, E], [0, 1, 2, 3], [1, 1, 1, 1], (4, 4, 0)),                 # all end-of-packet
    ([K, K, K], [0, 0, 0], [1, 0, 0], (0, 0, 3)),                          # no end-of-packet
    ([K, K, E], [0, 0, 0], [1, 0, 0], (1, 3, 0)),
    ([E, K], [0, 1], [1, 1], (1, 1, 1)),
    ([E, K, E, K, K], [0, 1, 1, 2, 2], [1, 1, 0, 1, 0], (2, 3, 2)),        # a trailing run
    ([E], [0], [1], (1, 1, 0)),                                            # a single record ...
    ([K], [0], [1], (0, 0, 1)),                                            # ... of each kind
    ([K | 1 << 16, E | 1 << 16, E | 6, K | 1 << 31, E], [0, 0, 1, 2, 2], [1, 0, 1, 1, 0], (3, 5, 0)),
    ([], [], [], (0, 0, 0)),
]


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_model_against_hand_written_rows(row):
    opts, pkt_of, heads, counts = ROWS[row]
    got = frag_model(np.array(opts, np.uint32))
    assert got[0].tolist() == pkt_of and got[0].dtype == np.uint32
    assert got[1].astype(int).tolist() == heads
    assert got[2] == counts
    w = walk(opts)
    assert (w[0], [int(h) for h in w[1]], w[2]) == (pkt_of, heads, counts)
    assert counts[1] + counts[2] == len(opts)


def test_model_against_the_walk_on_random_batches():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 1000):
        for p in (0.0, 0.3, 0.9, 1.0):
            opts = (rng.random(n) < p).astype(np.uint32) | (rng.integers(0, 4, n).astype(np.uint32) << 1)
            got, w = frag_model(opts), walk(opts)
            assert got[0].tolist() == w[0] and got[1].tolist() == w[1] and got[2] == w[2]

"""CPU tests of xfg_ring_egress (include/xdpfilter_gpu.h): the structure's
layout against the header, the symbol in both libraries, and every argument
check on a host-only context -- no GPU needed (no pointer is dereferenced
before the context is found to have no device)."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import pytest

import xfgpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
FIELDS = ["sz", "umem", "rx_descs", "rx_first", "rx_mask", "tx_descs", "tx_first", "tx_mask",
          "fill_addrs", "fill_first", "fill_mask", "count", "counts", "flags"]


def test_structure_matches_the_header(tmp_path):
    """sizeof and every offsetof, as the C compiler lays the header's
    structure out, against the binding's."""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    prints = "".join('printf("%s %%zu\\n", offsetof(struct xfg_egress, %s));\n' % (f, f)
                     for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\nprintf("sizeof %zu\\n", sizeof(struct xfg_egress));\n'
                   'printf("swap %u\\n", XFG_EGRESS_SWAP_MACS);\n' + prints + 'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert [name for name, _ in G.Egress._fields_] == FIELDS
    assert int(out["sizeof"]) == C.sizeof(G.Egress)
    for f in FIELDS:
        assert int(out[f]) == getattr(G.Egress, f).offset, f
    assert int(out["swap"]) == G.EGRESS_SWAP_MACS == 1


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbol_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, "xfg_ring_egress")
    assert "xfg_ring_egress" in G.EXPORTS


def good(**kw):
    """A well-formed request (pointers never dereferenced: a host-only
    context has no device)."""
    f = dict(sz=C.sizeof(G.Egress), umem=0x10000, rx_descs=0x20000, rx_first=0, rx_mask=0xffffffff,
             tx_descs=0x30000, tx_first=0, tx_mask=0xffffffff, fill_addrs=0x40000, fill_first=0,
             fill_mask=0xffffffff, count=1000, counts=0x50000, flags=0)
    f.update(kw)
    return G.Egress(**f)


def call(ctx, e, verdicts=0x60000):
    return G.lib.xfg_ring_egress(ctx, 0, None if e is None else C.byref(e), verdicts, None)


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


def test_host_only_context_is_enodev(host_only):
    f = host_only
    assert call(f.ctx, good()) == -errno.ENODEV
    assert call(f.ctx, good(flags=G.EGRESS_SWAP_MACS)) == -errno.ENODEV
    # the degenerate shapes that are allowed
    assert call(f.ctx, good(tx_descs=None), verdicts=None) == -errno.ENODEV
    assert call(f.ctx, good(fill_addrs=None)) == -errno.ENODEV
    assert call(f.ctx, good(umem=None)) == -errno.ENODEV
    assert call(f.ctx, good(count=0)) == -errno.ENODEV
    # rings of exactly count entries, a wrapping first
    assert call(f.ctx, good(count=1024, tx_mask=1023, fill_mask=1023, rx_mask=1023,
                            rx_first=0xfffffff0, tx_first=0xfffffff0,
                            fill_first=0xfffffff0)) == -errno.ENODEV
    assert call(f.ctx, good(count=2**32 - 1)) == -errno.ENODEV
    # a larger structure of a later version
    assert call(f.ctx, good(sz=C.sizeof(G.Egress) + 8)) == -errno.ENODEV
    with pytest.raises(OSError) as e:
        f.ring_egress(0x20000, 16, 0x60000, 0x50000, tx_ptr=0x30000, fill_ptr=0x40000)
    assert e.value.errno == errno.ENODEV


EINVAL_CASES = {
    "rx mask": dict(rx_mask=1000),
    "tx mask": dict(tx_mask=0xfffffffe),
    "fill mask": dict(fill_mask=6),
    "tx ring below count": dict(tx_mask=511),
    "fill ring below count": dict(fill_mask=511),
    "rx unaligned": dict(rx_descs=0x20004),
    "tx unaligned": dict(tx_descs=0x30004),
    "fill unaligned": dict(fill_addrs=0x40001),
    "counts unaligned": dict(counts=0x50004),
    "umem unaligned": dict(umem=0x10002),
    "count 2^32": dict(count=2**32),
    "no counts": dict(counts=None),
    "unknown flag": dict(flags=2),
    "unknown high flag": dict(flags=G.EGRESS_SWAP_MACS | 1 << 31),
    "swap without umem": dict(flags=G.EGRESS_SWAP_MACS, umem=None),
    "short structure": dict(sz=C.sizeof(G.Egress) - 1),
    "zero structure size": dict(sz=0),
    "no output ring": dict(tx_descs=None, fill_addrs=None),
    "no rx ring": dict(rx_descs=None),
}


@pytest.mark.parametrize("case", list(EINVAL_CASES))
def test_einval(host_only, case):
    assert call(host_only.ctx, good(**EINVAL_CASES[case])) == -errno.EINVAL


def test_einval_without_context_request_or_verdicts(host_only):
    assert call(None, good()) == -errno.EINVAL
    assert call(host_only.ctx, None) == -errno.EINVAL
    # verdicts are read whenever there is a TX ring
    assert call(host_only.ctx, good(), verdicts=None) == -errno.EINVAL
    with pytest.raises(OSError) as e:
        host_only.ring_egress(0x20000, 16, 0x60000, 0x50000)      # no output ring
    assert e.value.errno == errno.EINVAL

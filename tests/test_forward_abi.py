"""xfg_forward_egress's C ABI without a GPU: the symbol, the structures and
constants against the header, every -EINVAL on a host-only context, and -ENODEV
after them (no device pointer is touched before it)."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import pytest

import xfgpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
EINVAL, ENODEV = -errno.EINVAL, -errno.ENODEV
SYMBOLS = ["xfg_forward_egress", "xfg_fib_create", "xfg_fib_free", "xfg_fib_lookup_host"]


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbols_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in G.EXPORTS


FIELDS = {
    "xfg_fwd_port": (G.FwdPort, ["ifindex", "tx_descs", "tx_first", "tx_mask"]),
    "xfg_forward": (G.Forward, ["sz", "umem", "rx_descs", "rx_first", "rx_mask", "fib", "ports", "nports",
                                "stack", "fill_addrs", "fill_first", "fill_mask", "count", "counts",
                                "queue_of", "reason_of", "flags"]),
}
CONSTS = {"XFG_FWD_PORTS_MAX": G.FWD_PORTS_MAX, "XFG_FWD_REASONS": G.FWD_REASONS, "XFG_FWD_OK": G.FWD_OK,
          "XFG_FWD_NOT_IP": G.FWD_NOT_IP, "XFG_FWD_BAD_HDR": G.FWD_BAD_HDR, "XFG_FWD_TTL": G.FWD_TTL,
          "XFG_FWD_V6": G.FWD_V6, "XFG_FWD_NO_ROUTE": G.FWD_NO_ROUTE, "XFG_FWD_NH_RET": G.FWD_NH_RET,
          "XFG_FWD_FRAG": G.FWD_FRAG, "XFG_FWD_NO_PORT": G.FWD_NO_PORT}


def test_structures_and_constants_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    body = ""
    for st, (_, fields) in FIELDS.items():
        body += f'printf("{st}.sizeof %zu\\n", sizeof(struct {st}));\n'
        for f in fields:
            body += f'printf("{st}.{f} %zu\\n", offsetof(struct {st}, {f}));\n'
    for c in CONSTS:
        body += f'printf("{c} %u\\n", {c});\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\n' + body + 'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for st, (cls, fields) in FIELDS.items():
        assert int(out[st + ".sizeof"]) == C.sizeof(cls), st
        assert [n for n, _ in cls._fields_] == fields
        for f in fields:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, (st, f)
    for c, v in CONSTS.items():
        assert int(out[c]) == v, c
    assert (G.FWD_PORTS_MAX, G.FWD_REASONS) == (63, 9)


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


@pytest.fixture(scope="module")
def other_ctx():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


NH = [(5, 0, 0, bytes(6), bytes(6))]


@pytest.fixture(scope="module")
def fib(host_only):
    f = G.Fib(host_only, [(0, 0, 0)], NH)
    yield f
    f.free()


@pytest.fixture(scope="module")
def foreign_fib(other_ctx):
    f = G.Fib(other_ctx, [(0, 0, 0)], NH)
    yield f
    f.free()


def port(ifindex=5, tx_descs=0x30000, tx_first=0, tx_mask=0xffffffff):
    return G.FwdPort(ifindex, tx_descs, tx_first, tx_mask)


def forward(table, ports=None, **kw):
    ports = [port(5), port(6), port(7)] if ports is None else ports
    tab = G.fwd_ports(ports)
    f = dict(sz=C.sizeof(G.Forward), umem=0x10000, rx_descs=0x20000, rx_first=0, rx_mask=0xffffffff,
             fib=table.ptr, ports=tab, nports=len(ports), stack=G.SteerQueue(0x38000, 0, 0xffffffff),
             fill_addrs=0x40000, fill_first=0, fill_mask=0xffffffff, count=64, counts=0x50000,
             queue_of=0x70000, reason_of=0x78000, flags=0)
    f.update(kw)
    s = G.Forward(*[f[n] for n, _ in G.Forward._fields_])
    s._keep = tab
    return s


def call(ctx, s, verdicts=0x60000):
    return G.lib.xfg_forward_egress(ctx, 0, None if s is None else C.byref(s), verdicts, None)


GOOD = [
    dict(), dict(ports=[port()]), dict(ports=[port(1 + k) for k in range(63)]),
    dict(fill_addrs=None, fill_mask=5), dict(queue_of=None), dict(reason_of=None),
    dict(queue_of=None, reason_of=None),
    dict(rx_mask=63, rx_first=0xfffffff0, fill_mask=63, ports=[port(tx_mask=63, tx_first=60)],
         stack=G.SteerQueue(0x38000, 0xffffffff, 63)),
    dict(count=2**32 - 1), dict(count=0, umem=None, rx_descs=None), dict(sz=C.sizeof(G.Forward) + 8),
]


@pytest.mark.parametrize("k", range(len(GOOD)))
def test_host_only_context_is_enodev(host_only, fib, k):
    assert call(host_only.ctx, forward(fib, **GOOD[k])) == ENODEV


def test_empty_batch_needs_no_verdicts(host_only, fib):
    assert call(host_only.ctx, forward(fib, count=0), verdicts=None) == ENODEV


def test_host_only_binding_raises(host_only, fib):
    with pytest.raises(OSError) as e:
        host_only.forward_egress(0x10000, 0x20000, 64, 0x60000, 0x50000, fib, [(5, 0x30000), (6, 0x34000, 5, 63)],
                                 (0x38000, 0, 63))
    assert e.value.errno == errno.ENODEV


BAD = [
    dict(sz=C.sizeof(G.Forward) - 1), dict(sz=0),
    dict(fib=None),
    dict(nports=0), dict(ports=[port(1 + k) for k in range(64)]), dict(ports=None, nports=1),
    dict(ports=[port(), port(6, tx_descs=None)]),                      # a port without a ring
    dict(ports=[port(0)]), dict(ports=[port(5), port(6), port(5)]),    # ifindex 0, given twice
    dict(stack=G.SteerQueue(None, 0, 0xffffffff)),
    dict(flags=1), dict(flags=G.EGRESS_MULTIBUF), dict(flags=1 << 31),
    # the steer call's list, of the fields the two share
    dict(count=2**32), dict(counts=None), dict(counts=0x50004),
    dict(umem=None), dict(rx_descs=None), dict(umem=0x10004), dict(rx_descs=0x20004),
    dict(fill_addrs=0x40004),
    dict(rx_mask=5), dict(fill_mask=6),
    dict(ports=[port(tx_mask=5)]), dict(ports=[port(tx_descs=0x30004)]),
    dict(stack=G.SteerQueue(0x38000, 0, 5)), dict(stack=G.SteerQueue(0x38004, 0, 63)),
    dict(fill_mask=31), dict(ports=[port(tx_mask=31)]), dict(stack=G.SteerQueue(0x38000, 0, 31)),   # < count
]


@pytest.mark.parametrize("k", range(len(BAD)))
def test_refusals(host_only, fib, k):
    kw = dict(BAD[k])
    if "ports" in kw and kw["ports"] is None:
        s = forward(fib, **{a: b for a, b in kw.items() if a != "ports"})
        s.ports = None
    else:
        s = forward(fib, **kw)
    assert call(host_only.ctx, s) == EINVAL


def test_refusals_of_the_call_itself(host_only, fib, foreign_fib):
    assert call(None, forward(fib)) == EINVAL
    assert call(host_only.ctx, None) == EINVAL
    assert call(host_only.ctx, forward(fib), verdicts=None) == EINVAL
    assert call(host_only.ctx, forward(foreign_fib)) == EINVAL           # another context's FIB

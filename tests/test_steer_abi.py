"""CPU tests of xfg_steer_egress (include/xdpfilter_gpu.h): the symbol in both
libraries, the structures' layout and the constants against the header, and
every argument check on a host-only context (device pointers are made-up
numbers: none is dereferenced before the context is found to have no device;
the queue and avail tables are host memory and are read)."""
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


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbol_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, "xfg_steer_egress")
    assert "xfg_steer_egress" in G.EXPORTS


FIELDS = {
    "xfg_steer_queue": (G.SteerQueue, ["tx_descs", "tx_first", "tx_mask"]),
    "xfg_steer": (G.Steer, ["sz", "umem", "rx_descs", "rx_first", "rx_mask", "queues", "avail",
                            "nqueues", "navail", "mode", "skip_queue", "fill_addrs", "fill_first",
                            "fill_mask", "count", "counts", "queue_of", "flags"]),
}
CONSTS = {"XFG_STEER_QUEUES_MAX": G.STEER_QUEUES_MAX, "XFG_STEER_AVAIL_MAX": G.STEER_AVAIL_MAX,
          "XFG_STEER_L4_HASH": G.STEER_L4_HASH, "XFG_STEER_L4_SPORT": G.STEER_L4_SPORT,
          "XFG_STEER_L4_DPORT": G.STEER_L4_DPORT, "XFG_QUEUE_NONE": G.QUEUE_NONE}


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
    assert (G.STEER_QUEUES_MAX, G.STEER_AVAIL_MAX, G.QUEUE_NONE) == (64, 256, 0xff)
    assert G.Steer.sz.offset == 0


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


def queue(**kw):
    f = dict(tx_descs=0x30000, tx_first=0, tx_mask=0xffffffff)
    f.update(kw)
    return G.SteerQueue(f["tx_descs"], f["tx_first"], f["tx_mask"])


def steer(queues=None, avail=None, **kw):
    queues = [queue()] * 4 if queues is None else queues
    tab = G.steer_queues(queues)
    av = None if avail is None else (C.c_uint32 * max(len(avail), 1))(*avail)
    f = dict(sz=C.sizeof(G.Steer), umem=0x10000, rx_descs=0x20000, rx_first=0, rx_mask=0xffffffff,
             queues=tab, avail=av, nqueues=len(queues), navail=0 if avail is None else len(avail),
             mode=G.STEER_L4_HASH, skip_queue=0, fill_addrs=0x40000, fill_first=0,
             fill_mask=0xffffffff, count=64, counts=0x50000, queue_of=0x70000, flags=0)
    f.update(kw)
    s = G.Steer(*[f[n] for n, _ in G.Steer._fields_])
    s._keep = (tab, av)
    return s


def call(ctx, s, verdicts=0x60000):
    return G.lib.xfg_steer_egress(ctx, 0, None if s is None else C.byref(s), verdicts, None)


GOOD = [
    dict(),
    dict(queues=[queue()]),
    dict(queues=[queue()] * 64, skip_queue=63),
    dict(queues=[queue()] * 3, avail=[2, 2, 0, 1] * 64),                       # navail 256, weights
    dict(queues=[queue(), queue(tx_descs=None)], avail=[0]),                   # a queue nobody names
    dict(queues=[queue(), queue(tx_descs=0x30004, tx_mask=5)], avail=[0, 0]),  # ... is not looked at
    dict(mode=G.STEER_L4_SPORT), dict(mode=G.STEER_L4_DPORT),
    dict(fill_addrs=None, fill_mask=5), dict(queue_of=None), dict(flags=G.EGRESS_SWAP_MACS),
    dict(rx_mask=63, rx_first=0xfffffff0, fill_mask=63, queues=[queue(tx_mask=63, tx_first=60)] * 2),
    dict(count=2**32 - 1),
    dict(count=0, umem=None, rx_descs=None), dict(sz=C.sizeof(G.Steer) + 8),
    dict(avail=None, navail=1000),                                             # ignored without avail
]


@pytest.mark.parametrize("k", range(len(GOOD)))
def test_host_only_context_is_enodev(host_only, k):
    assert call(host_only.ctx, steer(**GOOD[k])) == ENODEV


def test_empty_batch_needs_no_verdicts(host_only):
    assert call(host_only.ctx, steer(count=0), verdicts=None) == ENODEV


def test_host_only_binding_raises(host_only):
    with pytest.raises(OSError) as e:
        host_only.steer_egress(0x10000, 0x20000, 64, 0x60000, 0x50000, [0x30000, (0x38000, 5, 63)],
                               avail=[1, 0, 1], mode=G.STEER_L4_DPORT, skip_queue=1)
    assert e.value.errno == errno.ENODEV


BAD = [
    dict(sz=C.sizeof(G.Steer) - 1), dict(sz=0),
    dict(nqueues=0), dict(queues=[queue()] * 65),
    dict(avail=[]), dict(avail=[0] * 257),                           # navail 0, above 256
    dict(avail=[0, 4]), dict(avail=[0, 1, 2, 3, 0xffffffff]),        # an entry >= nqueues
    dict(skip_queue=4), dict(skip_queue=0xffffffff),
    dict(mode=3), dict(mode=0xffffffff),
    dict(flags=G.EGRESS_MULTIBUF), dict(flags=G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS), dict(flags=2),
    dict(flags=1 << 31),
    dict(umem=None), dict(rx_descs=None), dict(counts=None), dict(count=0, counts=None),
    dict(umem=0x10004), dict(rx_descs=0x20004), dict(fill_addrs=0x40004), dict(counts=0x50004),
    dict(queues=[queue(), queue(tx_descs=0x30004)]),
    dict(rx_mask=62), dict(rx_mask=0x7ffffffe), dict(fill_mask=62), dict(count=0, rx_mask=5),
    dict(queues=[queue(), queue(tx_mask=62)]),
    dict(fill_mask=31), dict(queues=[queue(), queue(tx_mask=31)]),   # 64 records, rings of 32
    dict(queues=[queue(tx_mask=31), queue()], avail=[1], skip_queue=0),   # ... named by skip_queue alone
    dict(count=2**32), dict(count=2**40),
    dict(queues=[queue(), queue(tx_descs=None)]),                    # named by the identity table
    dict(queues=[queue(), queue(tx_descs=None)], avail=[0, 1]),
    dict(queues=[queue(), queue(tx_descs=None)], avail=[0], skip_queue=1),
    dict(queues=None, nqueues=4),
]


@pytest.mark.parametrize("k", range(len(BAD)))
def test_einval(host_only, k):
    kw = dict(BAD[k])
    if "queues" in kw and kw["queues"] is None:
        s = steer()
        s.queues = None
    else:
        s = steer(**kw)
    assert call(host_only.ctx, s) == EINVAL, kw


def test_einval_null_arguments(host_only):
    assert call(None, steer()) == EINVAL
    assert call(host_only.ctx, None) == EINVAL
    assert call(host_only.ctx, steer(), verdicts=None) == EINVAL


def test_a_refused_call_writes_nothing(host_only):
    for kw in (dict(mode=3), dict(avail=[0, 9]), dict(fill_mask=31)):
        s = steer(**kw)
        before = (bytes(s), bytes(s._keep[0]))
        assert call(host_only.ctx, s) == EINVAL
        assert (bytes(s), bytes(s._keep[0])) == before

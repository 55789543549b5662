"""CPU tests of xfg_capture / xfg_capture_descs (include/xdpfilter_gpu.h): the
structure's layout against the header, the symbols in both libraries, and
every argument check on a host-only context -- no GPU needed (no pointer is
dereferenced before the context is found to have no device)."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import pytest

import xfgpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
FIELDS = ["sz", "action_mask", "snaplen", "ts_ns", "ts0", "out", "out_bytes", "counts"]
DROP_MASK = 1 << 1


def test_structure_matches_the_header(tmp_path):
    """sizeof and every offsetof, as the C compiler lays the header's
    structure out, against the binding's."""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    prints = "".join('printf("%s %%zu\\n", offsetof(struct xfg_capture, %s));\n' % (f, f)
                     for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\nprintf("sizeof %zu\\n", sizeof(struct xfg_capture));\n'
                   + prints + 'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert [name for name, _ in G.Capture._fields_] == FIELDS
    assert int(out["sizeof"]) == C.sizeof(G.Capture)
    for f in FIELDS:
        assert int(out[f]) == getattr(G.Capture, f).offset, f


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
@pytest.mark.parametrize("sym", ["xfg_capture", "xfg_capture_descs"])
def test_symbols_in_both_libraries(name, sym):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, sym)
    assert sym in G.EXPORTS


def cap(**kw):
    """A well-formed request (pointers never dereferenced: a host-only
    context has no device)."""
    f = dict(sz=C.sizeof(G.Capture), action_mask=DROP_MASK, snaplen=0, ts_ns=0x70000, ts0=0,
             out=0x80000, out_bytes=1 << 20, counts=0x50000)
    f.update(kw)
    return G.Capture(**f)


def batch(**kw):
    f = dict(data=0x10000, offsets=None, lens=0x20000, count=1000, stride=64, lens_u16=0)
    f.update(kw)
    return G.Batch(**f)


def descs(**kw):
    f = dict(umem=0x10000, descs=0x20000, first=0, mask=0xffffffff, count=1000)
    f.update(kw)
    return G.DescBatch(**f)


def call(ctx, b, c, verdicts=0x60000):
    fn = G.lib.xfg_capture_descs if isinstance(b, G.DescBatch) else G.lib.xfg_capture
    return fn(ctx, 0, None if b is None else C.byref(b), verdicts,
              None if c is None else C.byref(c), None)


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


FORMS = {
    "stride 64": lambda: batch(),
    "stride 2048, u16 lengths": lambda: batch(stride=2048, lens_u16=1, lens=0x20002),
    "offsets": lambda: batch(offsets=0x30000, stride=0),
    "descriptor array": lambda: descs(),
    "descriptor ring, wrapping first": lambda: descs(mask=1023, first=0xfffffff0),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_host_only_context_is_enodev(host_only, form):
    ctx, b = host_only.ctx, FORMS[form]
    assert call(ctx, b(), cap()) == -errno.ENODEV
    # the allowed degenerate requests
    assert call(ctx, b(), cap(ts_ns=None, ts0=12345)) == -errno.ENODEV
    assert call(ctx, b(), cap(out=None, out_bytes=0)) == -errno.ENODEV
    assert call(ctx, b(), cap(out_bytes=51)) == -errno.ENODEV
    assert call(ctx, b(), cap(action_mask=0)) == -errno.ENODEV
    assert call(ctx, b(), cap(action_mask=0xffffffff, snaplen=96)) == -errno.ENODEV
    assert call(ctx, b(), cap(sz=C.sizeof(G.Capture) + 8)) == -errno.ENODEV   # a later version
    empty, full = b(), b()
    empty.count, full.count = 0, 2**32 - 1
    assert call(ctx, empty, cap(), verdicts=None) == -errno.ENODEV
    assert call(ctx, full, cap()) == -errno.ENODEV
    with pytest.raises(OSError) as e:
        host_only.capture_into(b(), 0x60000, DROP_MASK, 0x80000, 1 << 20, 0x50000)
    assert e.value.errno == errno.ENODEV


EINVAL_CAPTURE = {
    "short structure": dict(sz=C.sizeof(G.Capture) - 1),
    "zero structure size": dict(sz=0),
    "no counts": dict(counts=None),
    "no out with room": dict(out=None, out_bytes=4096),
    "out 8-byte aligned only": dict(out=0x80008),
    "out unaligned": dict(out=0x80001),
    "counts unaligned": dict(counts=0x50004),
    "ts_ns unaligned": dict(ts_ns=0x70004),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(EINVAL_CAPTURE))
def test_einval_request(host_only, form, case):
    assert call(host_only.ctx, FORMS[form](), cap(**EINVAL_CAPTURE[case])) == -errno.EINVAL


@pytest.mark.parametrize("form", list(FORMS))
def test_einval_verdicts_count_context(host_only, form):
    b = FORMS[form]
    assert call(host_only.ctx, b(), cap(), verdicts=None) == -errno.EINVAL
    big = b()
    big.count = 2**32
    assert call(host_only.ctx, big, cap()) == -errno.EINVAL
    assert call(None, b(), cap()) == -errno.EINVAL
    assert call(host_only.ctx, b(), None) == -errno.EINVAL


@pytest.mark.parametrize("mask", [1000, 6, 0xfffffffe])
def test_einval_ring_mask(host_only, mask):
    assert call(host_only.ctx, descs(mask=mask), cap()) == -errno.EINVAL


def test_einval_batches(host_only):
    """What the classify calls refuse of a batch."""
    ctx = host_only.ctx
    assert G.lib.xfg_capture(ctx, 0, None, 0x60000, C.byref(cap()), None) == -errno.EINVAL
    assert G.lib.xfg_capture_descs(ctx, 0, None, 0x60000, C.byref(cap()), None) == -errno.EINVAL
    assert call(ctx, batch(stride=0), cap()) == -errno.EINVAL
    assert call(ctx, batch(stride=72), cap()) == -errno.EINVAL
    assert call(ctx, batch(data=0x10008), cap()) == -errno.EINVAL
    assert call(ctx, batch(lens=None), cap()) == -errno.EINVAL
    assert call(ctx, descs(descs=None), cap()) == -errno.EINVAL
    assert call(ctx, descs(descs=0x20004), cap()) == -errno.EINVAL

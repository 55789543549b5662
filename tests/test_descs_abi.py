"""CPU tests of xfg_classify_descs_timed (include/xdpfilter_gpu.h): the symbol
in both libraries, and its argument checks on a host-only context -- no GPU
needed."""
import ctypes as C
import errno
import os

import pytest

import xfgpu as G

LIBDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xdp-tools_amd", "lib")


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbol_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, "xfg_classify_descs_timed")
    assert hasattr(lib, "xfg_classify_descs")


def call(ctx, db, verdicts, iters, ms):
    return G.lib.xfg_classify_descs_timed(ctx, 0, db, verdicts, iters, ms)


def test_host_only_context_and_argument_checks():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    ms = C.c_double()
    # (pointers never dereferenced: a host-only context has no device)
    good = G.DescBatch(0x1000, 0x1000, 0, 0xffffffff, 16)
    assert call(f.ctx, C.byref(good), 0x1000, 2, C.byref(ms)) == -errno.ENODEV
    with pytest.raises(OSError) as e:
        f.classify_descs_timed(0x1000, 0x1000, 16, 0x1000, 2)
    assert e.value.errno == errno.ENODEV
    # what xfg_classify_descs refuses with -EINVAL before it looks for a
    # device: no context, no batch, no verdict buffer for a non-empty batch
    assert call(None, C.byref(good), 0x1000, 2, C.byref(ms)) == -errno.EINVAL
    assert call(f.ctx, None, 0x1000, 2, C.byref(ms)) == -errno.EINVAL
    assert call(f.ctx, C.byref(good), None, 2, C.byref(ms)) == -errno.EINVAL
    for args in ((None, C.byref(good), 0x1000), (f.ctx, None, 0x1000), (f.ctx, C.byref(good), None)):
        assert G.lib.xfg_classify_descs(args[0], 0, args[1], args[2], None) == -errno.EINVAL
    assert G.lib.xfg_classify_descs(f.ctx, 0, C.byref(good), 0x1000, None) == -errno.ENODEV
    f.close()

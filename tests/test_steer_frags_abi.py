"""CPU tests of xfg_steer_frags_egress (include/xdpfilter_gpu.h): the symbol in
both libraries and every argument check on a host-only context.  The tables of
test_steer_abi.py -- what xfg_steer_egress accepts and refuses -- are run
against the new call, which differs in one flag: XFG_EGRESS_MULTIBUF is taken."""
import ctypes as C
import errno
import os

import pytest

import xfgpu as G
from test_steer_abi import BAD, GOOD, LIBDIR, host_only, steer  # noqa: F401  (host_only: a fixture)

EINVAL, ENODEV = -errno.EINVAL, -errno.ENODEV
MULTIBUF_ROWS = [k for k, kw in enumerate(BAD) if kw.get("flags", 0) in
                 (G.EGRESS_MULTIBUF, G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS)]
REFUSED = [k for k in range(len(BAD)) if k not in MULTIBUF_ROWS]


def call(ctx, s, verdicts=0x60000):
    return G.lib.xfg_steer_frags_egress(ctx, 0, None if s is None else C.byref(s), verdicts, None)


def call_single(ctx, s, verdicts=0x60000):
    return G.lib.xfg_steer_egress(ctx, 0, C.byref(s), verdicts, None)


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbol_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, "xfg_steer_frags_egress")
    assert "xfg_steer_frags_egress" in G.EXPORTS


def test_the_tables_have_the_rows_this_file_relies_on():
    assert len(MULTIBUF_ROWS) == 2 and len(REFUSED) == len(BAD) - 2
    flags = [kw["flags"] for kw in BAD if "flags" in kw]
    assert 2 in flags and 1 << 31 in flags


@pytest.mark.parametrize("k", range(len(GOOD)))
def test_host_only_context_is_enodev(host_only, k):
    """-ENODEV comes after the checks: everything xfg_steer_egress accepts."""
    assert call(host_only.ctx, steer(**GOOD[k])) == ENODEV


@pytest.mark.parametrize("flags", [G.EGRESS_MULTIBUF, G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS,
                                   G.EGRESS_SWAP_MACS, 0])
def test_multibuf_is_accepted(host_only, flags):
    assert call(host_only.ctx, steer(flags=flags)) == ENODEV


@pytest.mark.parametrize("flags", [2, 1 << 31, 2 | G.EGRESS_MULTIBUF, 1 << 31 | G.EGRESS_SWAP_MACS, 8,
                                   0xffffffff])
def test_other_flag_bits_are_refused(host_only, flags):
    assert call(host_only.ctx, steer(flags=flags)) == EINVAL


@pytest.mark.parametrize("k", REFUSED)
def test_einval(host_only, k):
    kw = dict(BAD[k])
    if "queues" in kw and kw["queues"] is None:
        s = steer()
        s.queues = None
    else:
        s = steer(**kw)
    assert call(host_only.ctx, s) == EINVAL, kw


def test_einval_before_enodev(host_only):
    """A bad argument on a host-only context is -EINVAL, a good call -ENODEV:
    the context is looked at last."""
    assert call(host_only.ctx, steer(mode=3, flags=G.EGRESS_MULTIBUF)) == EINVAL
    assert call(host_only.ctx, steer(flags=G.EGRESS_MULTIBUF)) == ENODEV


def test_einval_null_arguments(host_only):
    assert call(None, steer()) == EINVAL
    assert call(host_only.ctx, None) == EINVAL
    assert call(host_only.ctx, steer(), verdicts=None) == EINVAL


def test_empty_batch(host_only):
    """count == 0 needs no umem, records or verdicts, but its counts."""
    assert call(host_only.ctx, steer(count=0, umem=None, rx_descs=None), verdicts=None) == ENODEV
    assert call(host_only.ctx, steer(count=0, counts=None)) == EINVAL
    assert call(host_only.ctx, steer(count=0, rx_mask=5)) == EINVAL


def test_a_refused_call_writes_nothing(host_only):
    for kw in (dict(mode=3), dict(avail=[0, 9]), dict(fill_mask=31), dict(flags=2)):
        s = steer(**kw)
        before = (bytes(s), bytes(s._keep[0]))
        assert call(host_only.ctx, s) == EINVAL
        assert (bytes(s), bytes(s._keep[0])) == before


def test_host_only_binding_raises(host_only):
    with pytest.raises(OSError) as e:
        host_only.steer_frags_egress(0x10000, 0x20000, 64, 0x60000, 0x50000, [0x30000, (0x38000, 5, 63)],
                                     avail=[1, 0, 1], mode=G.STEER_L4_DPORT, skip_queue=1,
                                     flags=G.EGRESS_MULTIBUF)
    assert e.value.errno == errno.ENODEV


@pytest.mark.parametrize("k", MULTIBUF_ROWS)
def test_the_single_buffer_call_still_refuses_multibuf(host_only, k):
    assert call_single(host_only.ctx, steer(**BAD[k])) == EINVAL

"""CPU tests of xfg_forward_frags_egress (include/xdpfilter_gpu.h): the symbol
in both libraries and every argument check on a host-only context.  The tables
of test_forward_abi.py -- what xfg_forward_egress accepts and refuses -- are run
against the new call, which differs in one flag: XFG_EGRESS_MULTIBUF is taken."""
import ctypes as C
import errno
import os

import pytest

import xfgpu as G
from test_forward_abi import (BAD, GOOD, LIBDIR, fib, foreign_fib, forward, host_only,  # noqa: F401
                              other_ctx, port)                                          # (fixtures)

EINVAL, ENODEV = -errno.EINVAL, -errno.ENODEV
SYM = "xfg_forward_frags_egress"
MULTIBUF_ROWS = [k for k, kw in enumerate(BAD) if kw.get("flags", 0) == G.EGRESS_MULTIBUF]
REFUSED = [k for k in range(len(BAD)) if k not in MULTIBUF_ROWS]


def call(ctx, s, verdicts=0x60000):
    return getattr(G.lib, SYM)(ctx, 0, None if s is None else C.byref(s), verdicts, None)


def call_single(ctx, s, verdicts=0x60000):
    return G.lib.xfg_forward_egress(ctx, 0, C.byref(s), verdicts, None)


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbol_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, SYM)
    assert SYM in G.EXPORTS


def test_the_tables_have_the_rows_this_file_relies_on():
    assert len(MULTIBUF_ROWS) == 1 and len(REFUSED) == len(BAD) - 1
    flags = [kw["flags"] for kw in BAD if "flags" in kw]
    assert 1 in flags and 1 << 31 in flags


@pytest.mark.parametrize("k", range(len(GOOD)))
def test_host_only_context_is_enodev(host_only, fib, k):  # noqa: F811
    """-ENODEV comes after the checks: everything xfg_forward_egress accepts."""
    assert call(host_only.ctx, forward(fib, **GOOD[k])) == ENODEV


@pytest.mark.parametrize("flags", [G.EGRESS_MULTIBUF, 0])
def test_multibuf_is_accepted(host_only, fib, flags):  # noqa: F811
    assert call(host_only.ctx, forward(fib, flags=flags)) == ENODEV


@pytest.mark.parametrize("flags", [1, 2, 1 << 31, 1 | G.EGRESS_MULTIBUF, 2 | G.EGRESS_MULTIBUF,
                                   1 << 31 | G.EGRESS_MULTIBUF, 8, 0xffffffff])
def test_other_flag_bits_are_refused(host_only, fib, flags):  # noqa: F811
    """Bit 0 (XFG_EGRESS_SWAP_MACS: the rewrite sets both addresses), bit 1,
    bit 31, with and without the bit that is taken."""
    assert call(host_only.ctx, forward(fib, flags=flags)) == EINVAL


@pytest.mark.parametrize("k", REFUSED)
def test_einval(host_only, fib, k):  # noqa: F811
    kw = dict(BAD[k])
    if "ports" in kw and kw["ports"] is None:
        s = forward(fib, **{a: b for a, b in kw.items() if a != "ports"})
        s.ports = None
    else:
        s = forward(fib, **kw)
    assert call(host_only.ctx, s) == EINVAL, kw


def test_einval_before_enodev(host_only, fib):  # noqa: F811
    """A bad argument on a host-only context is -EINVAL, a good call -ENODEV:
    the context is looked at last."""
    assert call(host_only.ctx, forward(fib, rx_mask=5, flags=G.EGRESS_MULTIBUF)) == EINVAL
    assert call(host_only.ctx, forward(fib, flags=G.EGRESS_MULTIBUF)) == ENODEV


def test_einval_of_the_call_itself(host_only, fib, foreign_fib):  # noqa: F811
    assert call(None, forward(fib)) == EINVAL
    assert call(host_only.ctx, None) == EINVAL
    assert call(host_only.ctx, forward(fib), verdicts=None) == EINVAL
    assert call(host_only.ctx, forward(foreign_fib)) == EINVAL           # another context's FIB


def test_empty_batch(host_only, fib):  # noqa: F811
    """count == 0 needs no umem, records or verdicts, but its counts."""
    assert call(host_only.ctx, forward(fib, count=0, umem=None, rx_descs=None), verdicts=None) == ENODEV
    assert call(host_only.ctx, forward(fib, count=0, counts=None)) == EINVAL
    assert call(host_only.ctx, forward(fib, count=0, rx_mask=5)) == EINVAL


def test_a_refused_call_writes_nothing(host_only, fib):  # noqa: F811
    for kw in (dict(fill_mask=31), dict(flags=1), dict(ports=[port(0)])):
        s = forward(fib, **kw)
        before = (bytes(s), bytes(s._keep))
        assert call(host_only.ctx, s) == EINVAL
        assert (bytes(s), bytes(s._keep)) == before


def test_host_only_binding_raises(host_only, fib):  # noqa: F811
    with pytest.raises(OSError) as e:
        host_only.forward_frags_egress(0x10000, 0x20000, 64, 0x60000, 0x50000, fib,
                                       [(5, 0x30000), (6, 0x34000, 5, 63)], (0x38000, 0, 63),
                                       flags=G.EGRESS_MULTIBUF)
    assert e.value.errno == errno.ENODEV


@pytest.mark.parametrize("k", MULTIBUF_ROWS)
def test_the_single_buffer_call_still_refuses_multibuf(host_only, fib, k):  # noqa: F811
    assert call_single(host_only.ctx, forward(fib, **BAD[k])) == EINVAL

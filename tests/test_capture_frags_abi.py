"""CPU tests of xfg_capture_descs_frags (include/xdpfilter_gpu.h): the symbol in
both libraries and in the binding, the flags argument of its prototype, every
argument check on a host-only context -- no GPU needed (no pointer is
dereferenced before the context is found to have no device) -- and the packet
formation model of capfragmodel.py, its two statements against each other and
against hand-written rows."""
import ctypes as C
import errno
import os
import re

import numpy as np
import pytest

import capfragmodel as CM
import xfgpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
SYM = "xfg_capture_descs_frags"
DROP_MASK = 1 << 1


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbol_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    assert hasattr(lib, SYM)
    assert SYM in G.EXPORTS


def test_prototype_and_flag():
    """The header's declaration: flags is a uint32_t between cap and stream;
    the binding passes it as one, and its flag is the header's."""
    src = open(os.path.join(ROOT, "include", "xdpfilter_gpu.h")).read()
    m = re.search(r"int\s+xfg_capture_descs_frags\s*\(([^;]*)\)\s*;", src)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["xfg_ctx *ctx", "int dev", "const struct xfg_desc_batch *batch",
                    "const uint8_t *verdicts", "const struct xfg_capture *cap", "uint32_t flags",
                    "void *stream"]
    fn = getattr(G.lib, SYM)
    assert fn.restype is C.c_int
    assert fn.argtypes[5] is C.c_uint32 and len(fn.argtypes) == 7
    assert fn.argtypes[2]._type_ is G.DescBatch and fn.argtypes[4]._type_ is G.Capture
    flag = re.search(r"#define\s+XFG_CAPTURE_HEAD_ONLY\s+\(1u\s*<<\s*(\d+)\)", src)
    assert flag and G.CAPTURE_HEAD_ONLY == 1 << int(flag.group(1)) == 1


def cap(**kw):
    """A well-formed request (pointers never dereferenced: a host-only
    context has no device)."""
    f = dict(sz=C.sizeof(G.Capture), action_mask=DROP_MASK, snaplen=0, ts_ns=0x70000, ts0=0,
             out=0x80000, out_bytes=1 << 20, counts=0x50000)
    f.update(kw)
    return G.Capture(**f)


def descs(**kw):
    f = dict(umem=0x10000, descs=0x20000, first=0, mask=0xffffffff, count=1000)
    f.update(kw)
    return G.DescBatch(**f)


def call(ctx, b, c, verdicts=0x60000, flags=0):
    return getattr(G.lib, SYM)(ctx, 0, None if b is None else C.byref(b), verdicts,
                               None if c is None else C.byref(c), flags, None)


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


FORMS = {
    "descriptor array": lambda: descs(),
    "descriptor ring, wrapping first": lambda: descs(mask=1023, first=0xfffffff0),
}


@pytest.mark.parametrize("flags", [0, G.CAPTURE_HEAD_ONLY])
@pytest.mark.parametrize("form", list(FORMS))
def test_host_only_context_is_enodev(host_only, form, flags):
    """-ENODEV after the argument checks, for every request they allow --
    count == 0 and action_mask == 0 among them, as for the sibling calls."""
    ctx, b = host_only.ctx, FORMS[form]
    assert call(ctx, b(), cap(), flags=flags) == -errno.ENODEV
    assert call(ctx, b(), cap(ts_ns=None, ts0=12345), flags=flags) == -errno.ENODEV
    assert call(ctx, b(), cap(out=None, out_bytes=0), flags=flags) == -errno.ENODEV
    assert call(ctx, b(), cap(out_bytes=51), flags=flags) == -errno.ENODEV
    assert call(ctx, b(), cap(action_mask=0), flags=flags) == -errno.ENODEV
    assert call(ctx, b(), cap(action_mask=0xffffffff, snaplen=96), flags=flags) == -errno.ENODEV
    assert call(ctx, b(), cap(sz=C.sizeof(G.Capture) + 8), flags=flags) == -errno.ENODEV
    empty, full = b(), b()
    empty.count, full.count = 0, 2**32 - 1
    assert call(ctx, empty, cap(), verdicts=None, flags=flags) == -errno.ENODEV
    assert call(ctx, full, cap(), flags=flags) == -errno.ENODEV
    with pytest.raises(OSError) as e:
        host_only.capture_frags_into(b(), 0x60000, DROP_MASK, 0x80000, 1 << 20, 0x50000,
                                     flags=flags)
    assert e.value.errno == errno.ENODEV


@pytest.mark.parametrize("flags", [1 << 1, 0x80000000, 3, 0xfffffffe])
@pytest.mark.parametrize("form", list(FORMS))
def test_einval_flags(host_only, form, flags):
    assert call(host_only.ctx, FORMS[form](), cap(), flags=flags) == -errno.EINVAL
    with pytest.raises(OSError) as e:
        host_only.capture_frags_into(FORMS[form](), 0x60000, DROP_MASK, 0x80000, 1 << 20, 0x50000,
                                     flags=flags)
    assert e.value.errno == errno.EINVAL


# every -EINVAL of xfg_capture_descs (test_capture_abi.py)
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


@pytest.mark.parametrize("flags", [0, G.CAPTURE_HEAD_ONLY])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(EINVAL_CAPTURE))
def test_einval_request(host_only, form, case, flags):
    assert call(host_only.ctx, FORMS[form](), cap(**EINVAL_CAPTURE[case]),
                flags=flags) == -errno.EINVAL
    # the sibling refuses the same request
    assert G.lib.xfg_capture_descs(host_only.ctx, 0, C.byref(FORMS[form]()), 0x60000,
                                   C.byref(cap(**EINVAL_CAPTURE[case])), None) == -errno.EINVAL


@pytest.mark.parametrize("form", list(FORMS))
def test_einval_verdicts_count_context(host_only, form):
    b = FORMS[form]
    assert call(host_only.ctx, b(), cap(), verdicts=None) == -errno.EINVAL
    big = b()
    big.count = 2**32
    assert call(host_only.ctx, big, cap()) == -errno.EINVAL
    assert call(None, b(), cap()) == -errno.EINVAL
    assert call(host_only.ctx, b(), None) == -errno.EINVAL
    assert call(host_only.ctx, None, cap()) == -errno.EINVAL


@pytest.mark.parametrize("mask", [1000, 6, 0xfffffffe])
def test_einval_ring_mask(host_only, mask):
    assert call(host_only.ctx, descs(mask=mask), cap()) == -errno.EINVAL


def test_einval_batches(host_only):
    ctx = host_only.ctx
    assert call(ctx, descs(descs=None), cap()) == -errno.EINVAL
    assert call(ctx, descs(descs=0x20004), cap()) == -errno.EINVAL
    assert call(ctx, descs(umem=0x10008), cap()) == -errno.EINVAL


# ---- the packet formation model
C_, E, X = CM.CONTD, 0, CM.VERDICT_NONE   # an option word with / without CONTD; a NONE byte
DROP, PASS = 1, 2

# (options, verdict bytes, mask) -> (heads, ends (-1: not complete), selected heads)
ROWS = {
    "empty": ([], [], DROP_MASK, [], [], []),
    "singles": ([E, E, E], [DROP, PASS, DROP], DROP_MASK, [0, 1, 2], [0, 1, 2], [0, 2]),
    "one packet of three": ([C_, C_, E], [DROP, PASS, PASS], DROP_MASK, [0], [2], [0]),
    "the head's byte alone selects": ([C_, E, C_, E], [PASS, DROP, DROP, PASS], DROP_MASK,
                                      [0, 2], [1, 3], [2]),
    "a NONE record separates two runs": ([C_, E, E, C_, E], [DROP, DROP, X, DROP, 7], DROP_MASK,
                                         [0, 3], [1, 4], [0, 3]),
    "a run ends in CONTD before a NONE record": ([E, C_, C_, E, E], [DROP, DROP, DROP, X, DROP],
                                                 DROP_MASK, [0, 1, 4], [0, -1, 4], [0, 4]),
    "a run ends in CONTD at the end of the batch": ([C_, E, C_, C_], [DROP, 0, DROP, DROP],
                                                    DROP_MASK, [0, 2], [1, -1], [0]),
    "a NONE record in the middle of a run": ([C_, C_, C_, E, E], [DROP, DROP, X, DROP, DROP],
                                             DROP_MASK, [0, 3, 4], [-1, 3, 4], [3, 4]),
    "a NONE record's own options do not matter": ([C_, E, C_, E], [X, DROP, X, X], DROP_MASK,
                                                  [1], [1], [1]),
    "all NONE": ([E, C_, E], [X, X, X], CM.MASK_ALL, [], [], []),
    "bytes 32 and 254 are live and never selected": ([C_, E, E, C_, E], [32, DROP, 254, 31, 0],
                                                     CM.MASK_ALL, [0, 2, 3], [1, 2, 4], [3]),
    "other option bits are ignored": ([0x10000 | C_, 0xfffe, 2], [DROP, PASS, DROP], DROP_MASK,
                                      [0, 2], [1, 2], [0, 2]),
    "last record alone is CONTD": ([E, C_], [DROP, DROP], DROP_MASK, [0, 1], [0, -1], [0]),
}


@pytest.mark.parametrize("row", list(ROWS))
def test_model_rows(row):
    opts, v, mask, heads, ends, sel = ROWS[row]
    for f in (CM.form, CM.walk):
        h, e, c, s = f(np.array(opts, np.uint32), np.array(v, np.uint8), mask)
        assert list(h) == heads and list(e) == ends, f.__name__
        assert list(c) == [x >= 0 for x in ends], f.__name__
        assert [int(a) for a, b in zip(h, s) if b] == sel, f.__name__


@pytest.mark.parametrize("seed", range(8))
def test_model_statements_agree(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 400))
    opts = (rng.random(n) < [0.3, 0.6, 0.9][seed % 3]).astype(np.uint32) | \
        (rng.integers(0, 2**15, n).astype(np.uint32) << 1)
    v = np.array([0, 1, 2, 4, 31, 32, 254, 255], np.uint8)[rng.integers(0, 8, n)]
    v[rng.random(n) < 0.5] = 1
    mask = [DROP_MASK, 3, 1 << 4 | 1 << 31, CM.MASK_ALL][seed % 4]
    got, want = CM.form(opts, v, mask), CM.walk(opts, v, mask)
    for a, b in zip(got, want):
        assert a.tolist() == list(b)

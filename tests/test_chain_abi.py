"""CPU tests of the chained-stage calls (xfg_classify_chain,
xfg_classify_descs_chain, xfg_classify_descs_chain_timed;
include/xdpfilter_gpu.h): the symbols in both libraries, the structure's
layout against the header, the argument checks on a host-only context (every
refusal comes before the context is found to have no device, and no pointer is
dereferenced: the device pointers passed are garbage), the empty batch, and
the numpy model of the GPU tests against a per-frame loop."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import xfgpu as G
import chainmodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
SYMBOLS = ["xfg_classify_chain", "xfg_classify_descs_chain", "xfg_classify_descs_chain_timed"]
EINVAL, ENODEV = -errno.EINVAL, -errno.ENODEV


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbols_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in G.EXPORTS


def test_structure_and_constants_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    fields = ["sz", "chain_mask", "flags", "idx", "counts"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\n'
                   'printf("sizeof %zu\\n", sizeof(struct xfg_chain));\n' +
                   "".join('printf("%s %%zu\\n", offsetof(struct xfg_chain, %s));\n' % (f, f)
                           for f in fields) +
                   'printf("pass %u\\n", XFG_CHAIN_PASS);\n'
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(G.Chain)
    assert [name for name, _ in G.Chain._fields_] == fields
    for f in fields:
        assert int(out[f]) == getattr(G.Chain, f).offset, f
    assert int(out["pass"]) == G.CHAIN_PASS == 1 << 2


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


# garbage device pointers: never read
DATA, LENS, OFFS, DESCS, VERD, IDX = 0x10000, 0x20000, 0x30000, 0x40000, 0x60001, 0x70000


def chain(**kw):
    f = dict(sz=C.sizeof(G.Chain), chain_mask=G.CHAIN_PASS, flags=0, idx=IDX)
    f.update(kw)
    ch = G.Chain(f["sz"], f["chain_mask"], f["flags"], f["idx"])
    ch.counts[0] = ch.counts[1] = 0xA5
    return ch


def batch(count=1000, data=DATA, lens=LENS, offsets=None, stride=64, lens_u16=0):
    return G.Batch(data, offsets, lens, count, stride, lens_u16)


def dbatch(count=1000, umem=DATA, descs=DESCS, first=0, mask=0xffffffff):
    return G.DescBatch(umem, descs, first, mask, count)


def ref(x):
    return None if x is None else C.byref(x)


def call_b(ctx, b, ch, verdicts=VERD, dev=0):
    return G.lib.xfg_classify_chain(ctx, dev, ref(b), ref(ch), verdicts, None)


def call_d(ctx, db, ch, verdicts=VERD, dev=0):
    return G.lib.xfg_classify_descs_chain(ctx, dev, ref(db), ref(ch), verdicts, None)


def call_t(ctx, db, ch, verdicts=VERD, dev=0, ms=True):
    return G.lib.xfg_classify_descs_chain_timed(ctx, dev, ref(db), ref(ch), verdicts,
                                                (C.c_double * 3)() if ms else None)


CALLS = [(call_b, batch), (call_d, dbatch), (call_t, dbatch)]


@pytest.mark.parametrize("call,mk", CALLS, ids=["batch", "descs", "descs_timed"])
def test_einval_of_the_chain_arguments(host_only, call, mk):
    ctx = host_only.ctx
    assert call(None, mk(), chain()) == EINVAL
    assert call(ctx, None, chain()) == EINVAL
    assert call(ctx, mk(), None) == EINVAL
    assert call(ctx, mk(), chain(sz=C.sizeof(G.Chain) - 1)) == EINVAL
    assert call(ctx, mk(), chain(sz=0)) == EINVAL
    for flags in (1, 2, 1 << 31):
        assert call(ctx, mk(), chain(flags=flags)) == EINVAL
    for idx in (IDX + 1, IDX + 2, IDX + 3):
        assert call(ctx, mk(), chain(idx=idx)) == EINVAL
    assert call(ctx, mk(), chain(), verdicts=None) == EINVAL
    assert call(ctx, mk(count=2**32), chain()) == EINVAL
    assert call(ctx, mk(count=2**40), chain()) == EINVAL
    ch = chain(flags=1)
    assert call(ctx, mk(), ch) == EINVAL
    assert list(ch.counts) == [0xA5] * 2            # a refused call writes nothing


def test_einval_of_the_timed_call_without_ms(host_only):
    assert call_t(host_only.ctx, dbatch(), chain(), ms=False) == EINVAL


def test_einval_as_xfg_classify(host_only):
    ctx = host_only.ctx
    assert call_b(ctx, batch(data=None), chain()) == EINVAL
    assert call_b(ctx, batch(lens=None), chain()) == EINVAL
    assert call_b(ctx, batch(stride=0), chain()) == EINVAL
    assert call_b(ctx, batch(stride=72), chain()) == EINVAL           # no multiple of 16
    assert call_b(ctx, batch(data=DATA + 8), chain()) == EINVAL
    assert call_b(ctx, batch(data=DATA + 8, offsets=OFFS), chain()) == EINVAL
    assert call_b(ctx, batch(stride=0, offsets=OFFS), chain()) == ENODEV   # offsets: no stride needed
    # a fixed-stride batch whose offsets would not fit a descriptor's address field
    assert call_b(ctx, batch(count=2**32 - 1, stride=2**17), chain()) == EINVAL
    assert call_b(ctx, batch(count=2**31, stride=2**17), chain()) == ENODEV


def test_einval_as_xfg_classify_descs(host_only):
    ctx = host_only.ctx
    for call in (call_d, call_t):
        assert call(ctx, dbatch(umem=None), chain()) == EINVAL
        assert call(ctx, dbatch(descs=None), chain()) == EINVAL
        assert call(ctx, dbatch(descs=DESCS + 4), chain()) == EINVAL
        assert call(ctx, dbatch(mask=1000), chain()) == EINVAL        # no 2^k - 1
        assert call(ctx, dbatch(mask=1023, first=0xfffffff0), chain()) == ENODEV


@pytest.mark.parametrize("call,mk", CALLS, ids=["batch", "descs", "descs_timed"])
def test_host_only_context_is_enodev_after_the_checks(host_only, call, mk):
    ctx = host_only.ctx
    ch = chain()
    assert call(ctx, mk(), ch) == ENODEV
    assert list(ch.counts) == [0xA5] * 2
    assert call(ctx, mk(), chain(idx=None)) == ENODEV
    assert call(ctx, mk(), chain(chain_mask=0)) == ENODEV
    assert call(ctx, mk(), chain(chain_mask=0xffffffff)) == ENODEV
    assert call(ctx, mk(count=2**32 - 1), chain()) == ENODEV
    assert call(ctx, mk(), chain(sz=C.sizeof(G.Chain) + 8)) == ENODEV     # a later, longer structure
    assert call(ctx, mk(), chain(), dev=7) == ENODEV
    assert call(ctx, mk(), chain(flags=1), dev=7) == EINVAL               # the checks come first


def test_host_only_context_through_the_binding(host_only):
    f = host_only
    for fn, args in ((f.classify_chain, (DATA, LENS, 16, 64, VERD)),
                     (f.classify_descs_chain, (DATA, DESCS, 16, VERD)),
                     (f.classify_descs_chain_timed, (DATA, DESCS, 16, VERD))):
        with pytest.raises(OSError) as e:
            fn(*args)
        assert e.value.errno == errno.ENODEV


@pytest.mark.parametrize("call,mk", CALLS, ids=["batch", "descs", "descs_timed"])
def test_empty_batch(host_only, call, mk):
    """count == 0: {0, 0}, no device needed, no pointer needed."""
    ctx = host_only.ctx
    ch = chain()
    assert call(ctx, mk(count=0), ch) == 0
    assert list(ch.counts) == [0, 0]
    ch = chain(idx=None, chain_mask=0)
    assert call(ctx, mk(count=0), ch, verdicts=None) == 0
    assert list(ch.counts) == [0, 0]
    if mk is dbatch:       # as xfg_classify_descs: an empty batch's ring is not looked at
        ch = chain()
        assert call(ctx, G.DescBatch(None, None, 0, 1000, 0), ch, verdicts=None) == 0
        assert list(ch.counts) == [0, 0]
    assert call(ctx, mk(count=0), chain(flags=4)) == EINVAL
    assert host_only.classify_descs_chain(DATA, DESCS, 0, VERD) == (0, 0)
    assert host_only.classify_chain(DATA, LENS, 0, 64, VERD) == (0, 0)


# ---- the model
BYTES = [0, 1, 2, 3, 4, 31, 32, 0x80, 0xff]


@pytest.mark.parametrize("mask", [0, 1, 4, 5, 1 << 31, 1 << 3 | 1 << 4, 0xffffffff])
def test_model_against_the_walk(mask):
    rng = np.random.default_rng(mask % 1000 + 3)
    for n in (0, 1, 2, 65, 1000):
        v = np.array(BYTES, np.uint8)[rng.integers(0, len(BYTES), n)]
        lens = rng.integers(0, 400, n).astype(np.uint32)
        offs = (rng.permutation(n).astype(np.uint64) * np.uint64(512)) | (np.uint64(1) << np.uint64(40))
        idx, counts = M.chain_model(v, mask)
        assert idx.dtype == np.uint32 and counts == (len(idx), n - len(idx))
        new = rng.integers(0, 3, len(idx)).astype(np.uint8)
        for stride, offsets in ((160, None), (0, offs)):
            w_idx, w_descs, w_out = M.walk(v, mask, lens, stride, offsets, new)
            assert idx.tolist() == w_idx
            d = M.descs_of_batch(lens, idx, stride, offsets)
            assert [(int(a), int(l) & 0xffffffff, int(l) >> 32) for a, l in d] == w_descs
            assert M.merge(v, idx, new).tolist() == w_out
        rec = rng.integers(0, 2**63, (n, 2)).astype(np.uint64)
        np.testing.assert_array_equal(M.descs_of_records(rec, idx), rec[[i for i in w_idx]].reshape(-1, 2))


def test_model_hand_written():
    v = [2, 1, 0, 2, 0xff, 32, 31, 3]
    assert M.selected(v, 4).tolist() == [0, 3]
    assert M.selected(v, 5).tolist() == [0, 2, 3]
    assert M.selected(v, 0xffffffff).tolist() == [0, 1, 2, 3, 6, 7]
    assert M.selected(v, 1 << 31).tolist() == [6]
    assert M.selected(v, 0).tolist() == []
    d = M.descs_of_batch([10, 200, 30, 64, 0, 0, 0, 0], [1, 3], stride=64)
    assert d.tolist() == [[64, 64], [192, 64]]                   # the slot bounds its frame
    assert M.merge(v, [0, 3], [1, 0]).tolist() == [1, 1, 0, 0, 0xff, 32, 31, 3]

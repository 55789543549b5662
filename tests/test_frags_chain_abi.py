"""CPU tests of the chained stage over multi-buffer batches
(xfg_classify_descs_frags_chain, xfg_classify_descs_frags_chain_timed;
include/xdpfilter_gpu.h): the symbols in both libraries, the structure's layout
against the header, the argument checks on a host-only context (every refusal
comes before the context is found to have no device, and no pointer is
dereferenced: the device pointers passed are garbage), the empty batch, and
the numpy model of the GPU tests against hand-written rows and a
record-at-a-time walk."""
import ctypes as C
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import xfgpu as G
import fragchainmodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "xdp-tools_amd", "lib")
SYMBOLS = ["xfg_classify_descs_frags_chain", "xfg_classify_descs_frags_chain_timed"]
EINVAL, ENODEV = -errno.EINVAL, -errno.ENODEV


@pytest.mark.parametrize("name", ["libxdpfilter_gpu.so", "libxdpfilter_gpu_diag.so"])
def test_symbols_in_both_libraries(name):
    lib = C.CDLL(os.path.join(LIBDIR, name))
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in G.EXPORTS


def test_structure_matches_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    fields = ["sz", "chain_mask", "flags", "idx", "counts"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\n'
                   'int main(void) {\n'
                   'printf("sizeof %zu\\n", sizeof(struct xfg_frags_chain));\n'
                   'printf("ncounts %zu\\n", sizeof(((struct xfg_frags_chain *)0)->counts) / 8);\n' +
                   "".join('printf("%s %%zu\\n", offsetof(struct xfg_frags_chain, %s));\n' % (f, f)
                           for f in fields) +
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(G.FragsChain)
    assert [name for name, _ in G.FragsChain._fields_] == fields
    for f in fields:
        assert int(out[f]) == getattr(G.FragsChain, f).offset, f
    assert int(out["ncounts"]) == len(G.FragsChain().counts) == 3


@pytest.fixture(scope="module")
def host_only():
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, ndev=0)
    yield f
    f.close()


# garbage device pointers: never read
UMEM, DESCS, VERD, IDX = 0x10000, 0x40000, 0x60001, 0x70000


def chain(**kw):
    f = dict(sz=C.sizeof(G.FragsChain), chain_mask=G.CHAIN_PASS, flags=0, idx=IDX)
    f.update(kw)
    ch = G.FragsChain(f["sz"], f["chain_mask"], f["flags"], f["idx"])
    ch.counts[0] = ch.counts[1] = ch.counts[2] = 0xA5
    return ch


def dbatch(count=1000, umem=UMEM, descs=DESCS, first=0, mask=0xffffffff):
    return G.DescBatch(umem, descs, first, mask, count)


def ref(x):
    return None if x is None else C.byref(x)


def call_d(ctx, db, ch, verdicts=VERD, dev=0):
    return G.lib.xfg_classify_descs_frags_chain(ctx, dev, ref(db), ref(ch), verdicts, None)


def call_t(ctx, db, ch, verdicts=VERD, dev=0, ms=True):
    return G.lib.xfg_classify_descs_frags_chain_timed(ctx, dev, ref(db), ref(ch), verdicts,
                                                      (C.c_double * 3)() if ms else None)


CALLS = [call_d, call_t]
IDS = ["descs", "descs_timed"]


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_einval_of_the_chain_arguments(host_only, call):
    ctx = host_only.ctx
    assert call(None, dbatch(), chain()) == EINVAL
    assert call(ctx, None, chain()) == EINVAL
    assert call(ctx, dbatch(), None) == EINVAL
    assert call(ctx, dbatch(), chain(sz=C.sizeof(G.FragsChain) - 1)) == EINVAL      # sz too small
    assert call(ctx, dbatch(), chain(sz=C.sizeof(G.Chain))) == EINVAL               # the shorter structure
    assert call(ctx, dbatch(), chain(sz=0)) == EINVAL
    for flags in (1, 2, 1 << 31):
        assert call(ctx, dbatch(), chain(flags=flags)) == EINVAL
    for idx in (IDX + 1, IDX + 2, IDX + 3):                                        # misaligned idx
        assert call(ctx, dbatch(), chain(idx=idx)) == EINVAL
    assert call(ctx, dbatch(), chain(), verdicts=None) == EINVAL                    # NULL verdicts, count != 0
    assert call(ctx, dbatch(mask=1000), chain()) == EINVAL                          # no 2^k - 1
    assert call(ctx, dbatch(mask=0xfffffffe), chain()) == EINVAL
    assert call(ctx, dbatch(count=2**32), chain()) == EINVAL
    assert call(ctx, dbatch(count=2**40), chain()) == EINVAL
    ch = chain(flags=1)
    assert call(ctx, dbatch(), ch) == EINVAL
    assert list(ch.counts) == [0xA5] * 3            # a refused call writes nothing


def test_einval_of_the_timed_call_without_ms(host_only):
    assert call_t(host_only.ctx, dbatch(), chain(), ms=False) == EINVAL


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_einval_as_xfg_classify_descs(host_only, call):
    ctx = host_only.ctx
    assert call(ctx, dbatch(umem=None), chain()) == EINVAL
    assert call(ctx, dbatch(descs=None), chain()) == EINVAL
    assert call(ctx, dbatch(descs=DESCS + 4), chain()) == EINVAL
    assert call(ctx, dbatch(mask=1023, first=0xfffffff0), chain()) == ENODEV


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_host_only_context_is_enodev_after_the_checks(host_only, call):
    ctx = host_only.ctx
    ch = chain()
    assert call(ctx, dbatch(), ch) == ENODEV
    assert list(ch.counts) == [0xA5] * 3
    assert call(ctx, dbatch(), chain(idx=None)) == ENODEV
    assert call(ctx, dbatch(), chain(chain_mask=0)) == ENODEV
    assert call(ctx, dbatch(), chain(chain_mask=0xffffffff)) == ENODEV
    assert call(ctx, dbatch(count=2**32 - 1), chain()) == ENODEV
    assert call(ctx, dbatch(), chain(sz=C.sizeof(G.FragsChain) + 8)) == ENODEV     # a later, longer structure
    assert call(ctx, dbatch(), chain(), dev=7) == ENODEV
    assert call(ctx, dbatch(), chain(flags=1), dev=7) == EINVAL                    # the checks come first


def test_host_only_context_through_the_binding(host_only):
    f = host_only
    for fn in (f.classify_descs_frags_chain, f.classify_descs_frags_chain_timed):
        with pytest.raises(OSError) as e:
            fn(UMEM, DESCS, 16, VERD)
        assert e.value.errno == errno.ENODEV


@pytest.mark.parametrize("call", CALLS, ids=IDS)
def test_empty_batch(host_only, call):
    """count == 0: {0, 0, 0}, no device needed, no pointer needed."""
    ctx = host_only.ctx
    ch = chain()
    assert call(ctx, dbatch(count=0), ch) == 0
    assert list(ch.counts) == [0, 0, 0]
    ch = chain(idx=None, chain_mask=0)
    assert call(ctx, dbatch(count=0), ch, verdicts=None) == 0
    assert list(ch.counts) == [0, 0, 0]
    ch = chain()          # as xfg_classify_descs: an empty batch's ring is not looked at
    assert call(ctx, G.DescBatch(None, None, 0, 1000, 0), ch, verdicts=None) == 0
    assert list(ch.counts) == [0, 0, 0]
    assert call(ctx, dbatch(count=0), chain(flags=4)) == EINVAL
    assert host_only.classify_descs_frags_chain(UMEM, DESCS, 0, VERD) == (0, 0, 0)
    assert host_only.classify_descs_frags_chain_timed(UMEM, DESCS, 0, VERD) == ((0, 0, 0), (0.0, 0.0, 0.0))


# ---- the model
N = 0xff    # XFG_VERDICT_NONE
P, D = 2, 1
ROWS = [
    # options (bit 0: continued), verdict bytes, mask, idx, ends, counts
    ([0, 0, 0], [P, D, P], 4, [0, 2], [0, 2], (2, 2, 1)),
    ([1, 1, 0, 1, 0], [P, D, D, D, P], 4, [0], [2], (1, 3, 2)),                  # the head's byte alone
    ([1, 1, 0, 1, 0], [D, P, P, D, P], 4, [], [], (0, 0, 5)),
    ([1, 1, 0, 1, 0], [D, P, P, P, D], 6, [0, 3], [2, 4], (2, 5, 0)),
    ([1, 0, 1, 1], [P, P, P, P], 4, [0], [1], (1, 2, 2)),                        # no end before the batch's
    ([1, 1, 0, 0], [P, N, P, P], 4, [2, 3], [2, 3], (2, 2, 2)),                  # a run cut: no packet; a new head
    ([1, 0, 1, 0], [N, P, P, N], 4, [1], [1], (1, 1, 3)),                        # a head after 0xff; a cut run
    ([1, 1, 0], [N, N, N], 0xffffffff, [], [], (0, 0, 3)),
    ([0, 0, 0, 0, 0, 0], [3, 4, 31, 32, 0x80, 0], 1 << 4 | 1 << 31 | 1, [1, 2, 5], [1, 2, 5], (3, 3, 3)),
    ([1 | 6, 1 << 16, 0], [P, D, P], 4, [0, 2], [1, 2], (2, 3, 0)),              # other option bits ignored
    ([], [], 4, [], [], (0, 0, 0)),
]


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_model_hand_written(row):
    opts, v, mask, idx, ends, counts = ROWS[row]
    got_idx, got_ends, got_counts = M.frags_chain_model(opts, v, mask)
    assert got_idx.dtype == np.uint32
    assert (got_idx.tolist(), got_ends.tolist(), got_counts) == (idx, ends, counts)
    assert M.walk(opts, v, mask)[:3] == (idx, ends, counts)


def test_merge_hand_written():
    v = [P, D, D, N, P, P, D]
    assert M.merge(v, [0, 4], [2, 5], [0, 1]).tolist() == [0, 0, 0, N, 1, 1, D]
    assert M.merge(v, [], [], []).tolist() == v


BYTES = [0, 1, 2, 2, 2, 3, 4, 31, 32, 0x80, 0xff]


@pytest.mark.parametrize("mask", [0, 1, 4, 5, 1 << 31, 1 << 3 | 1 << 4, 0xffffffff])
def test_model_against_the_walk(mask):
    rng = np.random.default_rng(mask % 1000 + 3)
    for n in (0, 1, 2, 65, 1000):
        for p_contd in (0.0, 0.5, 0.9):
            v = np.array(BYTES, np.uint8)[rng.integers(0, len(BYTES), n)]
            opts = (rng.random(n) < p_contd).astype(np.uint32) | \
                (rng.integers(0, 2, n).astype(np.uint32) << 16)
            idx, ends, counts = M.frags_chain_model(opts, v, mask)
            assert counts[1] + counts[2] == n and counts[0] == len(idx) <= counts[1]
            new = rng.integers(0, 3, len(idx)).astype(np.uint8)
            w_idx, w_ends, w_counts, w_out = M.walk(opts, v, mask, new)
            assert (idx.tolist(), ends.tolist(), counts) == (w_idx, w_ends, w_counts)
            assert M.merge(v, idx, ends, new).tolist() == w_out
            rec = rng.integers(0, 2**63, (n, 2)).astype(np.uint64)
            np.testing.assert_array_equal(M.heads_of_records(rec, idx), rec[w_idx].reshape(-1, 2))


def test_model_of_single_record_packets_is_the_chain_model():
    """Every record an end-of-packet record, no XFG_VERDICT_NONE byte:
    xfg_classify_descs_chain's selection."""
    import chainmodel
    rng = np.random.default_rng(8)
    v = np.array([b for b in BYTES if b != 0xff], np.uint8)[rng.integers(0, len(BYTES) - 1, 500)]
    for mask in (4, 5, 0xffffffff):
        idx, ends, counts = M.frags_chain_model(np.zeros(500, np.uint32), v, mask)
        want, wc = chainmodel.chain_model(v, mask)
        np.testing.assert_array_equal(idx, want)
        np.testing.assert_array_equal(ends, want)
        assert counts == (wc[0], wc[0], wc[1])

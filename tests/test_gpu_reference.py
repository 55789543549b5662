"""Every classify kernel against the reference's own programs, compiled for
the host without modification (oracle/ref/), over the corpus of
tests/refcorpus.py.  Expected values come from xftools.run_reference alone:
no call to the CPU restatement.  Bit-exact: verdicts, every rule value and
the per-action stats, after one launch and after a second launch of the same
batch through the same filter (counters accumulate across launches).

Reads only oracle/_ref/*.so (built beside the product, never the reference
tree) and fails where they are absent: a skip would hide the whole file.

Each case asserts the kernel that ran (Filter.last_path).  The kinds are
reached as the other GPU files reach them; batch sizes:
  whole   the corpus as it is, 159,165 frames (more than the 65,536 + rule
          slots the hit log of the pipelined kernels needs, xfg_plan.c)
  f64     the frames of at most 64 bytes (81,978), tiled under a seeded
          permutation per repeat to 131,109 = 2^17 + 37: the same edge frames
          at many lane and tile positions, a ragged last tile
No batch exceeds 2^18 frames.
"""
import functools

import numpy as np
import pytest

import refcorpus as R
import xftools as X
from test_gpu import assert_same, gpu_values, make_filter
from test_gpu_descs import Dev, ring_of, umem_of

pytestmark = pytest.mark.gpu

VARIANTS = [v for v, _ in X.VARIANTS]
GENERAL, PIPE, IPV4, QT, ETH = 0, 1, 2, 5, 6


@pytest.fixture(scope="module")
def G():
    assert X.have_reference(), "oracle/_ref/libref_*.so missing: run the build (make -C oracle ref)"
    import xfgpu
    return xfgpu


# ---- batches (built once, read only)
@functools.lru_cache(maxsize=None)
def batch(name):
    """(data, lens, stride, offsets)"""
    whole = np.arange(len(R.corpus()[0]))
    if name == "off":
        data, offs, lens = R.pack_offsets(whole)
        return data, lens, 0, offs
    if name == "f64":
        idx = R.tiled(R.fits64(), 1 << 17)
        assert len(idx) == (1 << 17) + 37
        return R.pack(idx, 64) + (64, None)
    stride = {"s160": 160, "s128": 128}[name]
    assert len(whole) <= 1 << 18
    return R.pack(whole, stride) + (stride, None)


# ---- rule sets
def rules_of(tag):
    """all: the corpus's rules.  v4: its IPv4 and port rules only (the
    IPv4-key kernel's census).  eth: its Ethernet rules only.
    qt-<live>[-v6]: IPv4 rules with only the `live` lookups (src, dst, both)
    able to hit, 2,000 more keys so that the map is past the LDS counter
    cache (XFG_LOG_MIN_KEYS), the port rules, and the IPv6 rules or none."""
    rs = R.rules()
    none = X.RuleSet()
    if tag == "all":
        return rs
    if tag == "eth":
        rs.v4_keys, rs.v4_vals, rs.v6_keys, rs.v6_vals = none.v4_keys, none.v4_vals, none.v6_keys, none.v6_vals
        return rs
    rs.eth_keys, rs.eth_vals = none.eth_keys, none.eth_vals
    if tag == "v4":
        rs.v6_keys, rs.v6_vals = none.v6_keys, none.v6_vals
        return rs
    _, live, *v6 = tag.split("-")
    mask = {"src": 1, "dst": 2, "both": 3}[live]
    if not v6:
        rs.v6_keys, rs.v6_vals = none.v6_keys, none.v6_vals
    more = X.rand_keys(5150, 2000, 4)
    have = {bytes(k) for k in rs.v4_keys}
    more = np.array([k for k in more if bytes(k) not in have], np.uint8)
    rng = np.random.default_rng(5151)
    keys = np.vstack([rs.v4_keys, more])
    flags = np.concatenate([rs.v4_vals & np.uint64(3), rng.integers(1, 4, len(more)).astype(np.uint64)])
    flags &= np.uint64(mask)
    flags[flags == 0] = 4          # present, never matching (CHECK_MAP's mask test)
    if mask == 3:                  # (both: keep src-only, dst-only and both mixed)
        assert {1, 2, 3} <= set(flags.tolist())
    hits = np.concatenate([rs.v4_vals >> np.uint64(6), rng.integers(0, 50, len(more)).astype(np.uint64)])
    rs.v4_keys, rs.v4_vals = keys, flags | (hits << np.uint64(6))
    return rs


_expected = {}


def expected(variant, bname, rtag):
    """The reference over the batch, and over it again with the values and
    stats the first run left: ((v, rules, stats) after 1, after 2)."""
    key = (variant, bname, rtag)
    if key not in _expected:
        data, lens, stride, offs = batch(bname)
        one = X.run_reference(variant, data, lens, rules_of(rtag), stride=stride, offsets=offs)
        two = X.run_reference(variant, data, lens, one[1], stride=stride, offsets=offs,
                              stats=one[2].copy())
        _expected[key] = (one, two)
    return _expected[key]


def launch(f, bname, how, dev_batch):
    data, lens, stride, offs = batch(bname)
    if how == "host":
        return f.classify_host(data, lens, stride=stride, offsets=offs)
    if how == "descs":
        return dev_batch.classify(0, 0xffffffff)
    return f.run(data, lens, stride=stride, offsets=offs)


def explain(bname, got, want):
    """The first few frames whose verdicts differ, for the failure message."""
    data, lens, stride, offs = batch(bname)
    bad = np.nonzero(got != want)[0]
    out = [f"{len(bad)} of {len(want)} verdicts differ"]
    for i in bad[:6].tolist():
        o = int(offs[i]) if offs is not None else i * stride
        out.append(f"frame {i} lane {i % 64} len {lens[i]} got {got[i]} want {want[i]}: "
                   + data[o:o + int(lens[i])].tobytes().hex())
    return "\n".join(out)


# (kind, variant, batch, rules, how, filter options)
CASES = []
for v in VARIANTS:
    # the general kernel: frames at offsets, and the host path's header
    # windows at a 160-byte stride
    CASES += [(GENERAL, v, "off", "all", "run", {}), (GENERAL, v, "s160", "all", "host", {})]
for v in ("xdpfilt_dny_all", "xdpfilt_alw_all"):
    CASES += [(PIPE, v, "s128", "all", "run", dict(window=128)),
              (PIPE, v, "s160", "all", "run", dict(window=128)),
              (PIPE, v, "f64", "all", "run", {}),
              (PIPE, v, "s160", "all", "descs", dict(window=128, descs_min_packets=1)),
              (PIPE, v, "f64", "all", "descs", dict(descs_min_packets=1))]
for v in ("xdpfilt_dny_ip", "xdpfilt_alw_all"):
    CASES += [(IPV4, v, "f64", "v4", "run", {}), (IPV4, v, "s160", "v4", "run", dict(window=128))]
for v in ("xdpfilt_dny_all", "xdpfilt_alw_ip"):
    for live in ("src", "dst", "both"):
        for v6 in ("", "-v6"):
            qt = dict(qt_min_keys=1, ipv4_capacity=1 << 16)
            CASES += [(QT, v, "f64", f"qt-{live}{v6}", "run", qt),
                      (QT, v, "s160", f"qt-{live}{v6}", "run", dict(window=128, **qt))]
for v in ("xdpfilt_dny_eth", "xdpfilt_alw_eth"):
    CASES += [(ETH, v, "f64", "eth", "run", {}), (ETH, v, "s160", "eth", "run", {})]


def case_id(c):
    kind, v, bname, rtag, how, opts = c
    return f"k{kind}-{v[8:]}-{bname}-{rtag}-{how}" + ("-w128" if opts.get("window") == 128 else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernels_against_reference(G, case):
    kind, variant, bname, rtag, how, opts = case
    rules = rules_of(rtag)
    (v1, r1, s1), (v2, r2, s2) = expected(variant, bname, rtag)
    f = make_filter(G, variant, **opts)
    f.load_rules(rules)
    dev_batch = None
    if how == "descs":
        data, lens, stride, _ = batch(bname)
        umem, addr = umem_of(data, lens, stride, seed=len(lens))
        descs, _, _ = ring_of(addr, lens)
        dev_batch = Dev(f, umem, descs, len(lens))
    for want_v, want_r, want_s in ((v1, r1, s1), (v2, r2, s2)):
        got = launch(f, bname, how, dev_batch)
        assert f.last_path() == kind
        assert np.array_equal(got, want_v), explain(bname, got, want_v)
        assert_same(got, gpu_values(f, G, rules), f.stats(), want_v, want_r, want_s)
    f.close()


def test_every_kind_has_a_case():
    assert {c[0] for c in CASES} == {GENERAL, PIPE, IPV4, QT, ETH}


def test_smoke_batch_against_reference(G):
    """__graft_entry__.smoke()'s exact batch, expected values from the
    reference."""
    rules, pool = X.random_rules(1234, n4=500, n6=100, ne=20, nports=30)
    data, lens = X.gen_fuzz(99, 50000, 160, rules, pool)
    rv, rrules, rst = X.run_reference("xdpfilt_dny_all", data, lens, rules, stride=160)
    f = make_filter(G, "xdpfilt_dny_all")
    f.load_rules(rules)
    v = f.run(data, lens, stride=160)
    assert_same(v, gpu_values(f, G, rules), f.stats(), rv, rrules, rst)
    f.close()

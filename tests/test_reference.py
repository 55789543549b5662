"""The CPU restatement (oracle/xf_oracle.c) against the reference's own
programs, compiled for the host without modification (oracle/ref/, DESIGN.md
§2): all ten xdpfilt_*.c, compared on verdicts, every rule value and the
per-action stats, bit-exact.  Where the two differ the reference is right.

Skipped where the reference libraries were not built (no reference tree at
build time); the GPU file beside this one, test_gpu_reference.py, fails
instead.
"""
import numpy as np
import pytest

import kat
import refcorpus as R
import xftools as X
from test_kat_counters import corpus as kat_corpus

pytestmark = pytest.mark.skipif(not X.have_reference(),
                                reason="oracle/_ref/ not built (no reference tree)")

VARIANTS = [v for v, _ in X.VARIANTS]
FIELDS = ("ports", "v4_vals", "v6_vals", "eth_vals")


def assert_same(got, want):
    np.testing.assert_array_equal(got[0], want[0], err_msg="verdicts")
    for fld in FIELDS:
        np.testing.assert_array_equal(getattr(got[1], fld), getattr(want[1], fld), err_msg=fld)
    np.testing.assert_array_equal(got[2], want[2], err_msg="stats")


@pytest.fixture(scope="module")
def whole():
    """The whole corpus at a 160-byte stride, its rules, and the reference's
    results per variant (computed once, read only)."""
    data, lens = R.pack(np.arange(len(R.corpus()[0])))
    rules = R.rules()
    ref = {v: X.run_reference(v, data, lens, rules, stride=R.MAXLEN) for v in VARIANTS}
    return data, lens, rules, ref


@pytest.mark.parametrize("variant", VARIANTS)
def test_features_word(variant):
    assert X.reference(variant).ref_features() == X.VARIANT_FEATURES[variant]


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_on_corpus(whole, variant):
    data, lens, rules, ref = whole
    got = X.run_oracle(X.VARIANT_FEATURES[variant], data, lens, rules, stride=R.MAXLEN)
    assert_same(got, ref[variant])


@pytest.fixture(scope="module")
def fuzz():
    rules, pool = X.random_rules(4321, n4=300, n6=120, ne=30, nports=40)
    data, lens = X.gen_fuzz(17, 100_000, 160, rules, pool)
    return rules, data, lens


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_on_fuzz(fuzz, variant):
    rules, data, lens = fuzz
    want = X.run_reference(variant, data, lens, rules, stride=160)
    assert_same(X.run_oracle(X.VARIANT_FEATURES[variant], data, lens, rules, stride=160), want)
    assert len(np.unique(want[0])) == 3


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_and_reference_on_kat(variant):
    """Every kat.py frame under test_kat_counters.py's rules; and the rows that
    state a verdict for this program, with the counter each bumps, hold for
    the reference itself."""
    frames = [fr for _, fr, _ in kat.kat_frames()]
    stride = 256
    data = np.zeros((len(frames), stride), np.uint8)
    for i, fr in enumerate(frames):
        data[i, :len(fr)] = np.frombuffer(fr, np.uint8)
    lens = np.array([len(fr) for fr in frames], np.uint32)
    rules = kat.kat_rules()
    want = X.run_reference(variant, data.reshape(-1), lens, rules, stride=stride)
    assert_same(X.run_oracle(X.VARIANT_FEATURES[variant], data.reshape(-1), lens, rules,
                             stride=stride), want)
    data, lens, rules, verd, after, stats = kat_corpus(variant)
    assert_same(X.run_reference(variant, data, lens, rules, stride=256), (verd, after, stats))


def test_ref_run_layouts_agree(whole):
    """Stride against offsets (frames back to back at unaligned starts); the
    values accumulate in place over a second run."""
    _, _, rules, ref = whole
    idx = np.arange(len(R.corpus()[0]))
    odata, offs, olens = R.pack_offsets(idx)
    for variant in ("xdpfilt_dny_all", "xdpfilt_alw_ip", "xdpfilt_dny_eth"):
        got = X.run_reference(variant, odata, olens, rules, offsets=offs)
        assert_same(got, ref[variant])
        v2, r2, s2 = X.run_reference(variant, odata, olens, got[1], offsets=offs, stats=got[2].copy())
        np.testing.assert_array_equal(v2, ref[variant][0])
        np.testing.assert_array_equal(s2, 2 * ref[variant][2])
        r0 = rules.prepared()
        for fld in FIELDS:
            np.testing.assert_array_equal(getattr(r2, fld) - getattr(r0, fld),
                                          2 * (getattr(ref[variant][1], fld) - getattr(r0, fld)))


# ---- the corpus cannot quietly turn bland
# Which verdicts a category's frames can get from a program, by its features
# (xdp-filter/xdpfilt_prog.h:224-306).  A MISS is always possible.  A HIT needs
# a lookup the category's frames reach: Ethernet for all of them; an address
# lookup for every category with an IP or ARP header (ARP only with IPV4,
# :241; ICMPv6 only IPv6 addresses); a port lookup where UDP / TCP headers
# occur.  ABORTED needs a parse that fails: below 14 bytes for every program
# (parse_ethhdr; the Ethernet-only programs parse nothing else); for the
# others a cut or lie inside a header they parse: the udp category cuts only
# behind a whole IPv4 header, so only the UDP feature aborts it; the tcp
# category's doff 0 cuts an IPv6 frame right behind its IPv6 header, which
# skip_ip6hdrext's two-byte check refuses for every program that parses IPv6
# (parsing_helpers.h:144; every program but the Ethernet-only ones); ARP is
# parsed with IPV4 only; the runt category is cut at 0-14 bytes.
T, U, V6F, V4F, E = X.FEAT_TCP, X.FEAT_UDP, X.FEAT_IPV6, X.FEAT_IPV4, X.FEAT_ETHERNET
MIXED = T | U | V6F | V4F | E
HIT_NEEDS = dict(trunc=MIXED, byte=MIXED, vlan=MIXED, ipv4=MIXED, ipv6=MIXED,
                 icmp6=E | V6F, udp=E | V4F | V6F | U, tcp=E | V4F | V6F | T, arp=E | V4F, runt=E)
DEEP = T | U | V6F | V4F
ABORT_NEEDS = dict(trunc=None, byte=None, runt=None, vlan=DEEP, ipv4=DEEP, ipv6=DEEP, icmp6=DEEP,
                   udp=U, tcp=DEEP, arp=V4F)


@pytest.mark.parametrize("variant", VARIANTS)
def test_corpus_is_not_bland(whole, variant):
    verd = whole[3][variant][0]
    cats = R.corpus()[2]
    feats = X.VARIANT_FEATURES[variant]
    hit, miss = (2, 1) if feats & X.FEAT_DENY else (1, 2)
    share = np.bincount(verd, minlength=3) / len(verd)
    print(variant, "ABORTED/DROP/PASS share", np.round(share, 3))
    assert share.min() >= 0.05, share
    for c, name in enumerate(R.CATS):
        got = set(np.unique(verd[cats == c]).tolist())
        want = {miss}
        if feats & HIT_NEEDS[name]:
            want.add(hit)
        if ABORT_NEEDS[name] is None or feats & ABORT_NEEDS[name]:
            want.add(0)
        assert got == want, (name, got, want)


def test_corpus_shape():
    frames, lens, cats = R.corpus()
    assert max(map(len, frames)) <= R.MAXLEN and len(frames) < (1 << 18)
    assert (lens[R.fits64()] <= 64).all() and len(R.fits64()) > 10000
    assert len(np.unique(cats)) == len(R.CATS)
    t = R.tiled(R.fits64(), 1 << 17)
    assert (1 << 17) <= len(t) < (1 << 17) + 64 and len(t) % 64 == 37
    assert set(t.tolist()) == set(R.fits64().tolist())

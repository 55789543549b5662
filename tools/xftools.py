"""tools/xftools.py — test / bench tooling (NOT the product).

ctypes bindings for:
  * tools/libxfsynth.so        seeded synthetic traffic (workloads C2..C5, fuzz)
  * oracle/build/liboracle.so  our CPU restatement of the xdpfilt_* program
  * oracle/_ref/libref_*.so    the reference's own xdpfilt_*.c, compiled for the
                               host (oracle/ref/; tests only)
  * oracle/_ref/libref_cpumap.so  the reference's redirect-cpu programs, likewise

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use the
oracle binding, and only as the checker / the CPU baseline.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# XFG_LIB=asan: the sanitizer builds (make asan; tools/asan_suite.sh)
_ASAN = os.environ.get("XFG_LIB") == "asan"

FEAT_TCP, FEAT_UDP, FEAT_IPV6, FEAT_IPV4, FEAT_ETHERNET = 1, 2, 4, 8, 16
FEAT_ALL = 31
FEAT_ALLOW, FEAT_DENY = 32, 64
FLAG_SRC, FLAG_DST, FLAG_TCP, FLAG_UDP = 1, 2, 4, 8
COUNTER_SHIFT = 6

# xdp-filter/Makefile:3-6 order, with each program's _features word
# (xdp-filter/xdpfilt_prog.h:313-315 evaluated for each xdpfilt_*.c).
VARIANTS = [
    ("xdpfilt_dny_udp", FEAT_UDP | FEAT_DENY),
    ("xdpfilt_dny_tcp", FEAT_TCP | FEAT_DENY),
    ("xdpfilt_dny_ip", FEAT_IPV4 | FEAT_IPV6 | FEAT_DENY),
    ("xdpfilt_dny_eth", FEAT_ETHERNET | FEAT_DENY),
    ("xdpfilt_dny_all", FEAT_ALL | FEAT_DENY),
    ("xdpfilt_alw_udp", FEAT_UDP | FEAT_ALLOW),
    ("xdpfilt_alw_tcp", FEAT_TCP | FEAT_ALLOW),
    ("xdpfilt_alw_ip", FEAT_IPV4 | FEAT_IPV6 | FEAT_ALLOW),
    ("xdpfilt_alw_eth", FEAT_ETHERNET | FEAT_ALLOW),
    ("xdpfilt_alw_all", FEAT_ALL | FEAT_ALLOW),
]
VARIANT_FEATURES = dict(VARIANTS)

_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)


def ptr(a, t=_u8p):
    if a is None:
        return None
    return a.ctypes.data_as(t)


@dataclass
class RuleSet:
    """Rule maps in the reference's value encoding (hits << 6 | flags)."""
    ports: np.ndarray = field(default_factory=lambda: np.zeros(65536, np.uint64))
    v4_keys: np.ndarray = field(default_factory=lambda: np.zeros((0, 4), np.uint8))
    v4_vals: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint64))
    v6_keys: np.ndarray = field(default_factory=lambda: np.zeros((0, 16), np.uint8))
    v6_vals: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint64))
    eth_keys: np.ndarray = field(default_factory=lambda: np.zeros((0, 6), np.uint8))
    eth_vals: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint64))

    def copy(self) -> "RuleSet":
        return RuleSet(*(np.array(getattr(self, f), copy=True) for f in
                         ("ports", "v4_keys", "v4_vals", "v6_keys", "v6_vals",
                          "eth_keys", "eth_vals")))

    def prepared(self):
        """Contiguous arrays of the right dtypes (for ctypes)."""
        r = RuleSet(np.ascontiguousarray(self.ports, np.uint64),
                    np.ascontiguousarray(self.v4_keys, np.uint8).reshape(-1, 4),
                    np.ascontiguousarray(self.v4_vals, np.uint64),
                    np.ascontiguousarray(self.v6_keys, np.uint8).reshape(-1, 16),
                    np.ascontiguousarray(self.v6_vals, np.uint64),
                    np.ascontiguousarray(self.eth_keys, np.uint8).reshape(-1, 6),
                    np.ascontiguousarray(self.eth_vals, np.uint64))
        return r


def port_key(port: int) -> int:
    """Key of filter_ports for a host-order port: htons(port) as u32
    (xdp-filter/xdp-filter.c:634)."""
    return ((port & 0xff) << 8) | (port >> 8)


# ----------------------------------------------------------------- synth
_synth = None


def synth():
    global _synth
    if _synth is None:
        lib = C.CDLL(os.path.join(ROOT, "tools", "build-asan" if _ASAN else "", "libxfsynth.so"))
        lib.xfs_gen_workload.argtypes = [C.c_uint64, C.c_int, C.c_uint64, C.c_uint32,
                                         _u8p, _u32p, _u8p, C.c_uint32, _u8p, C.c_uint32,
                                         _u16p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.xfs_gen_fuzz.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, _u8p, _u32p,
                                     _u8p, C.c_uint32, _u8p, C.c_uint32, _u8p, C.c_uint32,
                                     _u16p, C.c_uint32]
        lib.xfs_rand_keys.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, _u8p]
        _synth = lib
    return _synth


def rand_keys(seed: int, n: int, keylen: int, distinct: bool = True) -> np.ndarray:
    out = np.zeros((n, keylen), np.uint8)
    if n:
        synth().xfs_rand_keys(seed, n, keylen, ptr(out))
    if distinct and n:
        # first occurrence of each key (a flat view sorts far faster than axis=0)
        flat = (out.view("<u4").ravel() if keylen == 4 else
                out.view(np.dtype((np.void, keylen))).ravel())
        _, idx = np.unique(flat, return_index=True)
        out = out[np.sort(idx)]
    return out


def gen_workload(seed, kind, n, stride, v4=None, v6=None, ports=None,
                 dst_permille=500, port_permille=250, bad_permille=10,
                 data=None, lens=None):
    """Synthetic batch for configuration C<kind>; returns (data u8[n*stride], lens u32[n])."""
    if data is None:
        data = np.zeros(n * stride, np.uint8)
    if lens is None:
        lens = np.zeros(n, np.uint32)
    v4 = np.ascontiguousarray(v4 if v4 is not None else np.zeros((0, 4), np.uint8), np.uint8)
    v6 = np.ascontiguousarray(v6 if v6 is not None else np.zeros((0, 16), np.uint8), np.uint8)
    ports = np.ascontiguousarray(ports if ports is not None else np.zeros(0, np.uint16), np.uint16)
    rc = synth().xfs_gen_workload(seed, kind, n, stride, ptr(data), ptr(lens, _u32p),
                                  ptr(v4), len(v4), ptr(v6), len(v6), ptr(ports, _u16p),
                                  len(ports), dst_permille, port_permille, bad_permille)
    if rc:
        raise ValueError("xfs_gen_workload failed (stride too small?)")
    return data, lens


C1_MACS = np.array([[2, 0, 0, 0, 0, i] for i in range(1, 9)], np.uint8)   # 02:00:00:00:00:0{1..8}


def c1_rules():
    """C1's rule set: the 8 MACs 02:00:00:00:00:0{1..8}, the
    first 4 dst rules, the last 4 src rules (`xdp-filter ether -m dst|src`)."""
    rules = RuleSet()
    rules.eth_keys = C1_MACS.copy()
    rules.eth_vals = np.array([2] * 4 + [1] * 4, np.uint64)
    return rules


def gen_c1(seed, n, stride=64, hit_permille=250, bad_permille=10, data=None, lens=None):
    """C1's traffic: 64 B Ethernet/IPv4/UDP frames with random MACs, a ruled
    MAC (where its rule tests it) in `hit_permille` of them, and the
    Appendix A malformed classes in `bad_permille`."""
    return gen_workload(seed, 1, n, stride, v6=C1_MACS, dst_permille=hit_permille,
                        port_permille=0, bad_permille=bad_permille, data=data, lens=lens)


def gen_fuzz(seed, n, stride=160, rules: RuleSet | None = None, port_pool=None):
    data = np.zeros(n * stride, np.uint8)
    lens = np.zeros(n, np.uint32)
    r = (rules or RuleSet()).prepared()
    ports = np.ascontiguousarray(port_pool if port_pool is not None else
                                 np.zeros(0, np.uint16), np.uint16)
    rc = synth().xfs_gen_fuzz(seed, n, stride, ptr(data), ptr(lens, _u32p),
                              ptr(r.v4_keys), len(r.v4_keys), ptr(r.v6_keys), len(r.v6_keys),
                              ptr(r.eth_keys), len(r.eth_keys), ptr(ports, _u16p), len(ports))
    if rc:
        raise ValueError("xfs_gen_fuzz failed")
    return data, lens


def random_rules(seed, n4=64, n6=32, ne=16, nports=24, flag_mode="any"):
    """Random rule set with random flag combinations (incl. src-only/dst-only
    and proto-restricted port rules).  Returns (RuleSet, port_pool)."""
    rng = np.random.default_rng(seed)

    def flags(n, ip=True):
        if flag_mode == "dst":
            return np.full(n, FLAG_DST, np.uint64)
        f = rng.integers(1, 16, n).astype(np.uint64)
        if ip:   # ip/ether rules carry src/dst only (xdp-filter.c:784-786)
            f = rng.integers(1, 4, n).astype(np.uint64)
        return f

    rs = RuleSet()
    rs.v4_keys = rand_keys(seed * 11 + 1, n4, 4)
    rs.v4_vals = flags(len(rs.v4_keys)) | (rng.integers(0, 1000, len(rs.v4_keys)).astype(np.uint64) << 6)
    rs.v6_keys = rand_keys(seed * 11 + 2, n6, 16)
    rs.v6_vals = flags(len(rs.v6_keys)) | (rng.integers(0, 1000, len(rs.v6_keys)).astype(np.uint64) << 6)
    rs.eth_keys = rand_keys(seed * 11 + 3, ne, 6)
    rs.eth_vals = flags(len(rs.eth_keys))
    pool = rng.choice(65536, nports, replace=False).astype(np.uint16)
    for p in pool:
        rs.ports[port_key(int(p))] = np.uint64(int(rng.integers(1, 16)) | (int(rng.integers(0, 50)) << 6))
    return rs, pool


# ----------------------------------------------------------------- oracle
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        lib = C.CDLL(os.path.join(ROOT, "oracle", "build-asan" if _ASAN else "build", "liboracle.so"))
        lib.xfo_map_new.restype = C.c_void_p
        lib.xfo_map_new.argtypes = [C.c_uint32, C.c_uint32, _u8p]
        lib.xfo_map_new_hashed.restype = C.c_void_p
        lib.xfo_map_new_hashed.argtypes = [C.c_uint32, C.c_uint32, _u8p, _u64p]
        lib.xfo_map_free.argtypes = [C.c_void_p]
        common = [C.c_uint32, _u8p, _u64p, C.c_uint32, C.c_void_p, C.c_int, C.c_uint64, _u64p]
        lib.xfo_run.argtypes = common + [C.c_void_p, _u64p, C.c_void_p, _u64p, C.c_void_p,
                                         _u64p, _u8p, _u64p]
        lib.xfo_run_mt.argtypes = common + [C.c_void_p, _u64p, C.c_uint32, C.c_void_p, _u64p,
                                            C.c_uint32, C.c_void_p, _u64p, C.c_uint32,
                                            _u8p, _u64p, C.c_int]
        _oracle = lib
    return _oracle


class OracleMaps:
    """Prebuilt exact-match indexes for a RuleSet (reusable across runs)."""

    def __init__(self, rules: RuleSet, hashed: bool = False):
        """hashed: add the hash index (one probe per lookup, the reference's
        BPF hash-map cost model: the CPU baseline); results are identical."""
        lib = oracle()
        self.rules = rules.prepared()
        r = self.rules
        if hashed:   # (the slots carry the rules' flags as they are now)
            self.m4 = lib.xfo_map_new_hashed(len(r.v4_keys), 4, ptr(r.v4_keys), ptr(r.v4_vals, _u64p))
            self.m6 = lib.xfo_map_new_hashed(len(r.v6_keys), 16, ptr(r.v6_keys), ptr(r.v6_vals, _u64p))
            self.me = lib.xfo_map_new_hashed(len(r.eth_keys), 6, ptr(r.eth_keys),
                                             ptr(r.eth_vals, _u64p))
        else:
            self.m4 = lib.xfo_map_new(len(r.v4_keys), 4, ptr(r.v4_keys))
            self.m6 = lib.xfo_map_new(len(r.v6_keys), 16, ptr(r.v6_keys))
            self.me = lib.xfo_map_new(len(r.eth_keys), 6, ptr(r.eth_keys))

    def __del__(self):
        try:
            lib = oracle()
            for m in (self.m4, self.m6, self.me):
                lib.xfo_map_free(m)
        except Exception:
            pass


def run_oracle(features, data, lens, rules: RuleSet, stride=0, offsets=None,
               nthreads=1, maps: OracleMaps | None = None, stats=None):
    """Run the CPU restatement; returns (verdicts, rules_after, stats[5,2])."""
    lib = oracle()
    maps = maps or OracleMaps(rules)
    r = rules.prepared().copy()
    n = len(lens)
    verdicts = np.zeros(n, np.uint8)
    st = np.zeros(10, np.uint64) if stats is None else stats.reshape(10)
    lens_u16 = lens.dtype == np.uint16
    lens = np.ascontiguousarray(lens)
    offs = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    if nthreads <= 1:
        rc = lib.xfo_run(features, ptr(data), ptr(offs, _u64p), stride, lens.ctypes.data,
                         int(lens_u16), n, ptr(r.ports, _u64p), maps.m4, ptr(r.v4_vals, _u64p),
                         maps.m6, ptr(r.v6_vals, _u64p), maps.me, ptr(r.eth_vals, _u64p),
                         ptr(verdicts), ptr(st, _u64p))
    else:
        rc = lib.xfo_run_mt(features, ptr(data), ptr(offs, _u64p), stride, lens.ctypes.data,
                            int(lens_u16), n, ptr(r.ports, _u64p),
                            maps.m4, ptr(r.v4_vals, _u64p), len(r.v4_vals),
                            maps.m6, ptr(r.v6_vals, _u64p), len(r.v6_vals),
                            maps.me, ptr(r.eth_vals, _u64p), len(r.eth_vals),
                            ptr(verdicts), ptr(st, _u64p), nthreads)
    if rc:
        raise RuntimeError("oracle run failed")
    return verdicts, r, st.reshape(5, 2)


# ----------------------------------------------------------------- reference
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
_ref_libs: dict = {}


def _ref_path(variant):
    return os.path.join(REF_DIR, "libref_" + variant.removeprefix("xdpfilt_") + ".so")


def have_reference() -> bool:
    """True when all ten host builds of the reference's programs are present."""
    return all(os.path.exists(_ref_path(v)) for v, _ in VARIANTS)


def reference(variant):
    """The host build of the reference's xdpfilt_<variant>.c (oracle/ref/)."""
    lib = _ref_libs.get(variant)
    if lib is None:
        lib = C.CDLL(_ref_path(variant))
        lib.ref_features.restype = C.c_uint32
        lib.ref_features.argtypes = []
        lib.ref_run.argtypes = [_u8p, _u64p, C.c_uint32, _u32p, C.c_uint64, _u64p,
                                _u8p, _u64p, C.c_uint32, _u8p, _u64p, C.c_uint32,
                                _u8p, _u64p, C.c_uint32, _u8p, _u64p]
        _ref_libs[variant] = lib
    return lib


def run_reference(variant, data, lens, rules: RuleSet, stride=0, offsets=None, stats=None):
    """Run the reference's own program `variant` ("xdpfilt_dny_all", ...);
    returns (verdicts, rules_after, stats[5,2]) as run_oracle does."""
    lib = reference(variant)
    r = rules.prepared().copy()
    n = len(lens)
    verdicts = np.zeros(n, np.uint8)
    st = np.zeros(10, np.uint64) if stats is None else stats.reshape(10)
    data = np.ascontiguousarray(data, np.uint8)
    lens = np.ascontiguousarray(lens, np.uint32)
    offs = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    rc = lib.ref_run(ptr(data), ptr(offs, _u64p), stride, ptr(lens, _u32p), n,
                     ptr(r.ports, _u64p),
                     ptr(r.v4_keys), ptr(r.v4_vals, _u64p), len(r.v4_vals),
                     ptr(r.v6_keys), ptr(r.v6_vals, _u64p), len(r.v6_vals),
                     ptr(r.eth_keys), ptr(r.eth_vals, _u64p), len(r.eth_vals),
                     ptr(verdicts), ptr(st, _u64p))
    if rc:
        raise RuntimeError("reference run failed (no arena below 4 GiB?)")
    return verdicts, r, st.reshape(5, 2)


# ----------------------------------------------------------------- reference, redirect-cpu
STEER_HASH, STEER_SPORT, STEER_DPORT = 0, 1, 2      # XFG_STEER_L4_*; ref_cpumap_harness.c's modes
XDP_ABORTED, XDP_PASS, XDP_REDIRECT = 0, 2, 4
_ref_cpumap = None


def _ref_cpumap_path():
    return os.path.join(REF_DIR, "libref_cpumap.so")


def have_reference_steer() -> bool:
    """True when the host build of the reference's redirect-cpu programs is present."""
    return os.path.exists(_ref_cpumap_path())


def reference_steer():
    """The host build of the reference's xdp_redirect_cpumap.bpf.c (oracle/ref/)."""
    global _ref_cpumap
    if _ref_cpumap is None:
        lib = C.CDLL(_ref_cpumap_path())
        lib.ref_cpumap_nr_cpus.restype = C.c_uint32
        lib.ref_cpumap_nr_cpus.argtypes = []
        lib.ref_cpumap_run.argtypes = [_u8p, _u64p, C.c_uint32, _u32p, C.c_uint64, C.c_uint32,
                                       _u32p, C.c_uint32, _u8p, _u32p, _u64p]
        _ref_cpumap = lib
    return _ref_cpumap


def run_reference_steer(data, lens, mode, avail, skip_queue=0, stride=0, offsets=None, rec=None):
    """Run the reference's cpumap_l4_hash / _sport / _dport (mode STEER_*) with
    cpus_available = avail and cpus_count = len(avail), in xfg_steer_egress's
    terms: returns (queue, refused), a queue number and a flag per frame.
    XDP_REDIRECT: the queue is the key the program redirected to.  XDP_PASS
    (parse_eth refused the frame): skip_queue, refused.  XDP_ABORTED -- an
    avail entry at or above nr_cpus, which xfg_steer_egress refuses with
    -EINVAL as an entry at or above nqueues -- must not occur and raises.
    rec (u64[2], optional) accumulates rx_cnt's processed and issue."""
    lib = reference_steer()
    n = len(lens)
    data = np.ascontiguousarray(data, np.uint8)
    lens = np.ascontiguousarray(lens, np.uint32)
    offs = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    av = np.ascontiguousarray(avail, np.uint32)
    rcs = np.zeros(n, np.uint8)
    keys = np.zeros(n, np.uint32)
    rec = np.zeros(2, np.uint64) if rec is None else rec
    if lib.ref_cpumap_run(ptr(data), ptr(offs, _u64p), stride, ptr(lens, _u32p), n, mode,
                          ptr(av, _u32p), len(av), ptr(rcs), ptr(keys, _u32p), ptr(rec, _u64p)):
        raise RuntimeError("reference run failed (mode, empty avail table, or no arena below 4 GiB)")
    redirect = rcs == XDP_REDIRECT
    if not (redirect | (rcs == XDP_PASS)).all():
        bad = int(np.flatnonzero(~(redirect | (rcs == XDP_PASS)))[0])
        raise RuntimeError(f"reference returned {int(rcs[bad])} for frame {bad}: an avail entry >= nr_cpus?")
    return np.where(redirect, keys, skip_queue).astype(np.uint32), ~redirect


# ----------------------------------------------------------------- reference, xdp-forward
FWD_FULL, FWD_DIRECT = 0, 1                         # ref_forward_harness.c's modes
# ref_forward_harness.c's stages: where a frame's run ended
(FWD_ST_EARLY, FWD_ST_NO_ROUTE, FWD_ST_NH_RET, FWD_ST_FRAG, FWD_ST_NO_PORT, FWD_ST_REDIRECT,
 FWD_ST_V6) = range(7)
FWD_STAGES = 7
_ref_forward = None


def _ref_forward_path():
    return os.path.join(REF_DIR, "libref_forward.so")


def have_reference_forward() -> bool:
    """True when the host build of the reference's xdp-forward program is present."""
    return os.path.exists(_ref_forward_path())


def reference_forward():
    """The host build of the reference's xdp_forward.bpf.c (oracle/ref/)."""
    global _ref_forward
    if _ref_forward is None:
        lib = C.CDLL(_ref_forward_path())
        lib.ref_forward_run.argtypes = [_u8p, _u64p, C.c_uint32, _u32p, C.c_uint64, C.c_uint32,
                                        _u32p, C.c_uint32, _u32p, _u8p, C.c_uint32, _u32p, C.c_uint32,
                                        _u8p, _u32p, _u8p, _u8p, C.c_uint32, _u32p]
        _ref_forward = lib
    return _ref_forward


def forward_tables(routes, nexthops):
    """(routes u32[r, 3], nh u32[h, 3], macs u8[h, 12]) as ref_forward_run takes
    them, from (prefix, len, nexthop) and (ifindex, mtu, ret, dmac, smac) tuples."""
    r = np.ascontiguousarray(np.asarray(routes, np.int64).reshape(-1, 3), np.uint32)
    nh = np.ascontiguousarray([[h[0], h[1], h[2]] for h in nexthops], np.uint32).reshape(-1, 3)
    macs = np.frombuffer(b"".join(bytes(h[3]) + bytes(h[4]) for h in nexthops), np.uint8).reshape(-1, 12)
    return r, nh, np.ascontiguousarray(macs)


def run_reference_forward(data, lens, routes, nexthops, ports, stride=0, offsets=None, mode=FWD_FULL):
    """Run the reference's xdp_fwd_fib_full (mode FWD_DIRECT: xdp_fwd_fib_direct)
    with the route list, next hops and xdp_tx_ports ifindex list given, in
    xfg_forward_egress's terms.  Returns (queue, stage, after, seen): queue[i]
    the position in ports of the key the program redirected frame i to, len(ports)
    (the stack ring) where it returned XDP_PASS; stage[i] FWD_ST_*; after u8[n,
    width] the frames' bytes when the program has run (zeros behind lens[i]);
    seen u32[n, 3] the family, tot_len and ipv4_dst the lookup was handed
    (0xffffffff where it was not called).  Any other return code, or a redirect
    to a key that is no port, raises."""
    lib = reference_forward()
    n = len(lens)
    data = np.ascontiguousarray(data, np.uint8)
    lens = np.ascontiguousarray(lens, np.uint32)
    offs = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    r, nh, macs = forward_tables(routes, nexthops)
    pt = np.ascontiguousarray(ports, np.uint32)
    width = max(int(lens.max()) if n else 0, 1)
    rcs = np.zeros(n, np.uint8)
    keys = np.zeros(n, np.uint32)
    stages = np.zeros(n, np.uint8)
    after = np.zeros((n, width), np.uint8)
    seen = np.zeros((n, 3), np.uint32)
    if lib.ref_forward_run(ptr(data), ptr(offs, _u64p), stride, ptr(lens, _u32p), n, mode,
                           ptr(r, _u32p), len(r), ptr(nh, _u32p), ptr(macs), len(nh),
                           ptr(pt, _u32p), len(pt), ptr(rcs), ptr(keys, _u32p), ptr(stages),
                           ptr(after), width, ptr(seen, _u32p)):
        raise RuntimeError("reference run failed (mode, a malformed route, or no arena below 4 GiB)")
    redirect = rcs == XDP_REDIRECT
    if not (redirect | (rcs == XDP_PASS)).all():
        bad = int(np.flatnonzero(~(redirect | (rcs == XDP_PASS)))[0])
        raise RuntimeError(f"reference returned {int(rcs[bad])} for frame {bad}")
    if (redirect != (stages == FWD_ST_REDIRECT)).any():
        raise RuntimeError("reference: XDP_REDIRECT and the redirect stage disagree")
    queue = np.full(n, len(pt), np.uint32)
    if redirect.any():
        order = np.argsort(pt, kind="stable")
        at = np.minimum(np.searchsorted(pt[order], keys[redirect]), len(pt) - 1)
        if (pt[order][at] != keys[redirect]).any():
            raise RuntimeError("reference redirected to a key that is no port")
        queue[redirect] = order[at]
    return queue, stages, after, seen

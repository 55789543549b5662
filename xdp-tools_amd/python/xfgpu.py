"""xfgpu — Python (ctypes) view of the xdp-filter GPU C ABI (include/xdpfilter_gpu.h).

The product is the C library xdp-tools_amd/lib/libxdpfilter_gpu.so; this
module is the thin binding the tests and bench.py drive it through.  It
mirrors the reference's operations on its pinned maps
(xdp-filter/xdp-filter.c:73-157): per-device values like per-CPU values,
negative-errno errors raised as OSError.

There is no fallback: if the library is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import errno
import os
import sys

# One HIP runtime per process: torch ships its own libamdhip64 with the same
# SONAME; loading torch first makes this library bind to that copy instead of
# loading a second runtime next to it.
try:  # pragma: no cover - environment dependent
    import torch  # noqa: F401
except Exception:  # torch absent: the library uses /opt/rocm's runtime
    pass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# XFG_LIB=diag selects the diagnostics build (measurement knobs; tools/, and the
# test that lowers the QT fold threshold),
# XFG_LIB=asan the sanitizer build of the host C (the CPU suite under
# tools/asan_suite.sh)
# tools/ A/B runs may also name a library file outright (XFG_LIB=/path/x.so);
# a named file that is missing, or an unknown name, is an error (never the
# product library in its place)
_LIBS = {"diag": ("lib", "libxdpfilter_gpu_diag.so"), "asan": ("lib-asan", "libxdpfilter_gpu.so")}
_SEL = os.environ.get("XFG_LIB", "")
if _SEL.endswith(".so"):
    if not os.path.isfile(_SEL):
        raise ImportError(f"XFG_LIB names {_SEL!r}, which does not exist")
    LIB_PATH = _SEL
elif _SEL and _SEL not in _LIBS:
    raise ImportError(f"XFG_LIB={_SEL!r}: expected 'diag', 'asan' or a path to a .so")
else:
    LIB_PATH = os.path.join(os.path.dirname(HERE), *_LIBS.get(_SEL, ("lib", "libxdpfilter_gpu.so")))

FEAT_TCP, FEAT_UDP, FEAT_IPV6, FEAT_IPV4, FEAT_ETHERNET = 1, 2, 4, 8, 16
FEAT_ALL = 31
FEAT_ALLOW, FEAT_DENY = 32, 64
MAP_PORTS, MAP_IPV4, MAP_IPV6, MAP_ETHERNET = 0, 1, 2, 3
KEYLEN = {MAP_PORTS: 4, MAP_IPV4: 4, MAP_IPV6: 16, MAP_ETHERNET: 6}
ACTION_MAX = 5

# Every symbol include/xdpfilter_gpu.h declares (checked by the CPU tests).
EXPORTS = [
    "xfg_select_program", "xfg_open", "xfg_close", "xfg_prog_name", "xfg_prog_features",
    "xfg_num_devices", "xfg_strerror", "xfg_map_lookup", "xfg_map_update", "xfg_map_delete",
    "xfg_map_get_next_key", "xfg_map_count", "xfg_map_update_batch", "xfg_map_lookup_batch", "xfg_classify",
    "xfg_classify_host", "xfg_stats_read", "xfg_stats_read_dev", "xfg_stats_reset",
    "xfg_sync", "xfg_dev_alloc", "xfg_dev_free", "xfg_memcpy_h2d", "xfg_memcpy_d2h",
    "xfg_host_alloc_pinned", "xfg_host_free_pinned", "xfg_classify_timed", "xfg_stream_read_timed",
    "xfg_comm_unique_id", "xfg_comm_init", "xfg_comm_allreduce", "xfg_map_update_batch_percpu",
    "xfg_classify_descs", "xfg_compact", "xfg_classify_xsk_host", "xfg_host_register",
    "xfg_host_unregister", "xfg_last_path", "xfg_host_threads", "xfg_classify_descs_timed",
    "xfg_ring_egress", "xfg_capture", "xfg_capture_descs", "xfg_classify_descs_frags",
    "xfg_classify_descs_frags_timed", "xfg_classify_socks", "xfg_socks_egress",
    "xfg_classify_socks_frags", "xfg_socks_frags_egress", "xfg_capture_descs_frags",
    "xfg_classify_chain", "xfg_classify_descs_chain", "xfg_classify_descs_chain_timed",
    "xfg_classify_descs_frags_chain", "xfg_classify_descs_frags_chain_timed",
    "xfg_steer_egress", "xfg_steer_frags_egress",
    "xfg_fib_create", "xfg_fib_free", "xfg_fib_lookup_host", "xfg_forward_egress",
    "xfg_forward_frags_egress",
]
CAPTURE_HEAD_ONLY = 1        # XFG_CAPTURE_HEAD_ONLY
SOCKS_MAX = 1024
VERDICT_NONE = 0xff          # XFG_VERDICT_NONE
PKT_NONE = 0xffffffff        # XFG_PKT_NONE
EGRESS_SWAP_MACS = 1
EGRESS_MULTIBUF = 4
STEER_QUEUES_MAX, STEER_AVAIL_MAX = 64, 256      # XFG_STEER_QUEUES_MAX, XFG_STEER_AVAIL_MAX
STEER_L4_HASH, STEER_L4_SPORT, STEER_L4_DPORT = 0, 1, 2
QUEUE_NONE = 0xff            # XFG_QUEUE_NONE
FIB_NEXTHOPS_MAX, FIB_GROUPS_MAX = 32767, 32768  # XFG_FIB_NEXTHOPS_MAX, XFG_FIB_GROUPS_MAX
FWD_PORTS_MAX, FWD_REASONS = 63, 9               # XFG_FWD_PORTS_MAX, XFG_FWD_REASONS
(FWD_OK, FWD_NOT_IP, FWD_BAD_HDR, FWD_TTL, FWD_V6, FWD_NO_ROUTE, FWD_NH_RET, FWD_FRAG,
 FWD_NO_PORT) = range(9)
XDP_PKT_CONTD = 1
XDP_ABORTED, XDP_DROP, XDP_PASS = 0, 1, 2
CHAIN_PASS = 1 << XDP_PASS   # XFG_CHAIN_PASS
# include/xdpfilter_io.h
IO_EXPORTS = [
    "xfg_pcap_read", "xfg_host_batch_free", "xfg_pcapng_write_verdicts", "xfg_store_map_name",
    "xfg_store_has_map", "xfg_store_create_map", "xfg_store_remove_map", "xfg_store_map_capacity",
    "xfg_store_load", "xfg_store_save", "xfg_store_stats_read", "xfg_store_stats_write",
    "xfg_store_stats_remove", "xfg_pcapng_write_captured", "xfg_pcapng_begin", "xfg_pcapng_append",
]


class OpenOpts(C.Structure):
    _fields_ = [("sz", C.c_size_t), ("features", C.c_uint32),
                ("devices", C.POINTER(C.c_int)), ("ndev", C.c_int),
                ("ipv4_capacity", C.c_uint32), ("ipv6_capacity", C.c_uint32),
                ("eth_capacity", C.c_uint32), ("hash_seed", C.c_uint32),
                ("qt_min_keys", C.c_uint32), ("window", C.c_uint32), ("reserved0", C.c_uint32),
                ("descs_min_packets", C.c_uint32)]


class Batch(C.Structure):
    _fields_ = [("data", C.c_void_p), ("offsets", C.c_void_p), ("lens", C.c_void_p),
                ("count", C.c_uint64), ("stride", C.c_uint32), ("lens_u16", C.c_uint32)]


class StatsRecord(C.Structure):
    _fields_ = [("packets", C.c_uint64), ("bytes", C.c_uint64)]


class DescBatch(C.Structure):
    _fields_ = [("umem", C.c_void_p), ("descs", C.c_void_p), ("first", C.c_uint32),
                ("mask", C.c_uint32), ("count", C.c_uint64)]


class Egress(C.Structure):
    """struct xfg_egress (xfg_ring_egress)."""
    _fields_ = [("sz", C.c_size_t), ("umem", C.c_void_p),
                ("rx_descs", C.c_void_p), ("rx_first", C.c_uint32), ("rx_mask", C.c_uint32),
                ("tx_descs", C.c_void_p), ("tx_first", C.c_uint32), ("tx_mask", C.c_uint32),
                ("fill_addrs", C.c_void_p), ("fill_first", C.c_uint32), ("fill_mask", C.c_uint32),
                ("count", C.c_uint64), ("counts", C.c_void_p), ("flags", C.c_uint32)]


class SteerQueue(C.Structure):
    """struct xfg_steer_queue: one worker's TX ring."""
    _fields_ = [("tx_descs", C.c_void_p), ("tx_first", C.c_uint32), ("tx_mask", C.c_uint32)]


class Steer(C.Structure):
    """struct xfg_steer (xfg_steer_egress)."""
    _fields_ = [("sz", C.c_size_t), ("umem", C.c_void_p),
                ("rx_descs", C.c_void_p), ("rx_first", C.c_uint32), ("rx_mask", C.c_uint32),
                ("queues", C.POINTER(SteerQueue)), ("avail", C.POINTER(C.c_uint32)),
                ("nqueues", C.c_uint32), ("navail", C.c_uint32),
                ("mode", C.c_uint32), ("skip_queue", C.c_uint32),
                ("fill_addrs", C.c_void_p), ("fill_first", C.c_uint32), ("fill_mask", C.c_uint32),
                ("count", C.c_uint64), ("counts", C.c_void_p), ("queue_of", C.c_void_p),
                ("flags", C.c_uint32)]


class FibNexthop(C.Structure):
    """struct xfg_fib_nexthop."""
    _fields_ = [("ifindex", C.c_uint32), ("mtu", C.c_uint16), ("ret", C.c_uint8),
                ("dmac", C.c_uint8 * 6), ("smac", C.c_uint8 * 6)]


class FibRoute(C.Structure):
    """struct xfg_fib_route: prefix in host order."""
    _fields_ = [("prefix", C.c_uint32), ("nexthop", C.c_uint32), ("len", C.c_uint8)]


class FwdPort(C.Structure):
    """struct xfg_fwd_port: one egress port and its TX ring."""
    _fields_ = [("ifindex", C.c_uint32), ("tx_descs", C.c_void_p), ("tx_first", C.c_uint32),
                ("tx_mask", C.c_uint32)]


class Forward(C.Structure):
    """struct xfg_forward (xfg_forward_egress)."""
    _fields_ = [("sz", C.c_size_t), ("umem", C.c_void_p),
                ("rx_descs", C.c_void_p), ("rx_first", C.c_uint32), ("rx_mask", C.c_uint32),
                ("fib", C.c_void_p), ("ports", C.POINTER(FwdPort)), ("nports", C.c_uint32),
                ("stack", SteerQueue),
                ("fill_addrs", C.c_void_p), ("fill_first", C.c_uint32), ("fill_mask", C.c_uint32),
                ("count", C.c_uint64), ("counts", C.c_void_p), ("queue_of", C.c_void_p),
                ("reason_of", C.c_void_p), ("flags", C.c_uint32)]


def fib_routes(routes):
    """A ctypes array of FibRoute from (prefix, len, nexthop) triples (prefix in
    host order) or an (n, 3) integer array of them."""
    a = np.asarray(routes, np.int64).reshape(-1, 3)
    arr = (FibRoute * max(len(a), 1))()
    v = np.zeros(len(a), np.dtype([("prefix", "<u4"), ("nexthop", "<u4"), ("len", "u1")],
                                  align=True))
    v["prefix"], v["len"], v["nexthop"] = a[:, 0], a[:, 1], a[:, 2]
    assert v.dtype.itemsize == C.sizeof(FibRoute)
    C.memmove(arr, v.ctypes.data, v.nbytes)
    return arr


def fib_nexthops(nexthops):
    """A ctypes array of FibNexthop from (ifindex, mtu, ret, dmac, smac) tuples,
    the MACs six bytes each."""
    arr = (FibNexthop * max(len(nexthops), 1))()
    for i, (ifindex, mtu, ret, dmac, smac) in enumerate(nexthops):
        arr[i] = FibNexthop(ifindex, mtu, ret, (C.c_uint8 * 6)(*bytes(dmac)),
                            (C.c_uint8 * 6)(*bytes(smac)))
    return arr


def fwd_ports(ports):
    """A host port table (a ctypes array of FwdPort) from FwdPort values or
    (ifindex, tx_ptr[, tx_first, tx_mask]) tuples; without the last two the
    ring is a plain array."""
    arr = (FwdPort * max(len(ports), 1))()
    for i, p in enumerate(ports):
        if isinstance(p, FwdPort):
            arr[i] = p
        elif len(p) == 2:
            arr[i] = FwdPort(p[0], p[1], 0, 0xffffffff)
        else:
            arr[i] = FwdPort(*p)
    return arr


def steer_queues(queues):
    """A host queue table (a ctypes array of SteerQueue) from SteerQueue values
    or (tx_ptr, tx_first, tx_mask) triples; a bare pointer is a plain array."""
    arr = (SteerQueue * max(len(queues), 1))()
    for i, q in enumerate(queues):
        if isinstance(q, SteerQueue):
            arr[i] = q
        elif isinstance(q, (tuple, list)):
            arr[i] = SteerQueue(*q)
        else:
            arr[i] = SteerQueue(q, 0, 0xffffffff)
    return arr


class Frags(C.Structure):
    """struct xfg_frags (xfg_classify_descs_frags)."""
    _fields_ = [("sz", C.c_size_t), ("pkt_of", C.c_void_p), ("counts", C.c_uint64 * 3)]


class Chain(C.Structure):
    """struct xfg_chain (xfg_classify_chain, xfg_classify_descs_chain)."""
    _fields_ = [("sz", C.c_size_t), ("chain_mask", C.c_uint32), ("flags", C.c_uint32),
                ("idx", C.c_void_p), ("counts", C.c_uint64 * 2)]


class FragsChain(C.Structure):
    """struct xfg_frags_chain (xfg_classify_descs_frags_chain)."""
    _fields_ = [("sz", C.c_size_t), ("chain_mask", C.c_uint32), ("flags", C.c_uint32),
                ("idx", C.c_void_p), ("counts", C.c_uint64 * 3)]


class Sock(C.Structure):
    """struct xfg_sock: one socket's peeked RX batch, its TX ring, its fill ring."""
    _fields_ = [("rx_descs", C.c_void_p), ("rx_first", C.c_uint32), ("rx_mask", C.c_uint32),
                ("tx_descs", C.c_void_p), ("tx_first", C.c_uint32), ("tx_mask", C.c_uint32),
                ("fill_addrs", C.c_void_p), ("fill_first", C.c_uint32), ("fill_mask", C.c_uint32),
                ("count", C.c_uint32)]


class Socks(C.Structure):
    """struct xfg_socks (xfg_classify_socks, xfg_socks_egress)."""
    _fields_ = [("sz", C.c_size_t), ("umem", C.c_void_p), ("socks", C.POINTER(Sock)),
                ("flat", C.c_void_p), ("nsocks", C.c_uint32)]


class SocksEgress(C.Structure):
    """struct xfg_socks_egress (xfg_socks_egress)."""
    _fields_ = [("sz", C.c_size_t), ("fill_addrs", C.c_void_p), ("fill_first", C.c_uint32),
                ("fill_mask", C.c_uint32), ("counts", C.c_void_p), ("flags", C.c_uint32)]


class SocksFrags(C.Structure):
    """struct xfg_socks_frags (xfg_classify_socks_frags)."""
    _fields_ = [("sz", C.c_size_t), ("done", C.POINTER(C.c_uint32)), ("pkt_of", C.c_void_p),
                ("counts", C.c_uint64 * 3)]


def sock_table(socks):
    """A host socket table (a ctypes array of Sock) from Sock values or dicts of their
    fields; masks left out are 0xffffffff (plain arrays)."""
    arr = (Sock * max(len(socks), 1))()
    for i, s in enumerate(socks):
        if isinstance(s, Sock):
            arr[i] = s
            continue
        f = dict(rx_mask=0xffffffff, tx_mask=0xffffffff, fill_mask=0xffffffff)
        f.update(s)
        arr[i] = Sock(**f)
    return arr


class Capture(C.Structure):
    """struct xfg_capture (xfg_capture, xfg_capture_descs)."""
    _fields_ = [("sz", C.c_size_t), ("action_mask", C.c_uint32), ("snaplen", C.c_uint32),
                ("ts_ns", C.c_void_p), ("ts0", C.c_uint64), ("out", C.c_void_p),
                ("out_bytes", C.c_uint64), ("counts", C.c_void_p)]


class HostBatch(C.Structure):
    _fields_ = [("data", C.c_void_p), ("offsets", C.POINTER(C.c_uint64)),
                ("lens", C.POINTER(C.c_uint32)), ("orig_lens", C.POINTER(C.c_uint32)),
                ("ts_ns", C.POINTER(C.c_uint64)), ("count", C.c_uint64), ("bytes", C.c_uint64),
                ("linktype", C.c_uint32), ("pad", C.c_uint32)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built (run `make` at the repo root)")
    lib = C.CDLL(LIB_PATH)
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    sig = {
        "xfg_select_program": (C.c_int, [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32)]),
        "xfg_open": (C.c_int, [C.POINTER(vp), C.POINTER(OpenOpts)]),
        "xfg_close": (None, [vp]),
        "xfg_prog_name": (C.c_char_p, [vp]),
        "xfg_prog_features": (C.c_uint32, [vp]),
        "xfg_num_devices": (C.c_int, [vp]),
        "xfg_strerror": (C.c_char_p, [C.c_int]),
        "xfg_last_path": (C.c_int, [vp, C.c_int]),
        "xfg_map_lookup": (C.c_int, [vp, C.c_int, vp, u64p]),
        "xfg_map_update": (C.c_int, [vp, C.c_int, vp, u64p]),
        "xfg_map_delete": (C.c_int, [vp, C.c_int, vp]),
        "xfg_map_get_next_key": (C.c_int, [vp, C.c_int, vp, vp]),
        "xfg_map_count": (C.c_int64, [vp, C.c_int]),
        "xfg_map_update_batch": (C.c_int, [vp, C.c_int, vp, u64p, C.c_uint64]),
        "xfg_map_update_batch_percpu": (C.c_int, [vp, C.c_int, vp, u64p, C.c_uint64]),
        "xfg_pcap_read": (C.c_int, [C.c_char_p, C.POINTER(HostBatch)]),
        "xfg_host_batch_free": (None, [C.POINTER(HostBatch)]),
        "xfg_pcapng_write_verdicts": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(HostBatch),
                                                C.POINTER(C.c_uint8)]),
        "xfg_pcapng_write_captured": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(HostBatch),
                                                C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32]),
        "xfg_pcapng_begin": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint32]),
        "xfg_pcapng_append": (C.c_int, [C.c_char_p, vp, C.c_uint64]),
        "xfg_store_map_name": (C.c_char_p, [C.c_int]),
        "xfg_store_has_map": (C.c_int, [C.c_char_p, C.c_int]),
        "xfg_store_create_map": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32]),
        "xfg_store_remove_map": (C.c_int, [C.c_char_p, C.c_int]),
        "xfg_store_map_capacity": (C.c_int64, [C.c_char_p, C.c_int]),
        "xfg_store_load": (C.c_int, [vp, C.c_char_p]),
        "xfg_store_save": (C.c_int, [vp, C.c_char_p]),
        "xfg_store_stats_read": (C.c_int, [C.c_char_p, C.POINTER(StatsRecord)]),
        "xfg_store_stats_write": (C.c_int, [C.c_char_p, C.POINTER(StatsRecord)]),
        "xfg_store_stats_remove": (C.c_int, [C.c_char_p]),
        "xfg_map_lookup_batch": (C.c_int64, [vp, C.c_int, vp, C.c_uint64, u64p,
                                             C.POINTER(C.c_uint8)]),
        "xfg_classify": (C.c_int, [vp, C.c_int, C.POINTER(Batch), vp, vp]),
        "xfg_classify_host": (C.c_int, [vp, C.c_int, C.POINTER(Batch), vp]),
        "xfg_classify_descs": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch), vp, vp]),
        "xfg_classify_descs_frags": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch),
                                               C.POINTER(Frags), vp, vp]),
        "xfg_classify_descs_frags_timed": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch),
                                                     C.POINTER(Frags), vp,
                                                     C.POINTER(C.c_double)]),
        "xfg_classify_chain": (C.c_int, [vp, C.c_int, C.POINTER(Batch), C.POINTER(Chain), vp, vp]),
        "xfg_classify_descs_chain": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch),
                                               C.POINTER(Chain), vp, vp]),
        "xfg_classify_descs_chain_timed": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch),
                                                     C.POINTER(Chain), vp,
                                                     C.POINTER(C.c_double)]),
        "xfg_classify_descs_frags_chain": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch),
                                                     C.POINTER(FragsChain), vp, vp]),
        "xfg_classify_descs_frags_chain_timed": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch),
                                                           C.POINTER(FragsChain), vp,
                                                           C.POINTER(C.c_double)]),
        "xfg_classify_xsk_host": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch), C.c_uint64, vp]),
        "xfg_host_register": (C.c_int, [vp, vp, C.c_size_t]),
        "xfg_host_unregister": (C.c_int, [vp, vp]),
        "xfg_host_threads": (C.c_int, []),
        "xfg_compact": (C.c_int, [vp, C.c_int, vp, C.c_uint64, C.c_uint32, vp, vp, vp]),
        "xfg_ring_egress": (C.c_int, [vp, C.c_int, C.POINTER(Egress), vp, vp]),
        "xfg_classify_socks": (C.c_int, [vp, C.c_int, C.POINTER(Socks), vp, vp]),
        "xfg_steer_egress": (C.c_int, [vp, C.c_int, C.POINTER(Steer), vp, vp]),
        "xfg_steer_frags_egress": (C.c_int, [vp, C.c_int, C.POINTER(Steer), vp, vp]),
        "xfg_fib_create": (C.c_int, [vp, C.c_int, C.POINTER(FibRoute), C.c_uint64,
                                     C.POINTER(FibNexthop), C.c_uint32, C.POINTER(vp)]),
        "xfg_fib_free": (None, [vp]),
        "xfg_fib_lookup_host": (C.c_int, [vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "xfg_forward_egress": (C.c_int, [vp, C.c_int, C.POINTER(Forward), vp, vp]),
        "xfg_forward_frags_egress": (C.c_int, [vp, C.c_int, C.POINTER(Forward), vp, vp]),
        "xfg_socks_egress": (C.c_int, [vp, C.c_int, C.POINTER(Socks), C.POINTER(SocksEgress), vp,
                                       vp]),
        "xfg_classify_socks_frags": (C.c_int, [vp, C.c_int, C.POINTER(Socks),
                                               C.POINTER(SocksFrags), vp, vp]),
        "xfg_socks_frags_egress": (C.c_int, [vp, C.c_int, C.POINTER(Socks),
                                             C.POINTER(SocksEgress), C.POINTER(C.c_uint32), vp,
                                             vp]),
        "xfg_capture":(C.c_int, [vp, C.c_int, C.POINTER(Batch), vp, C.POINTER(Capture), vp]),
        "xfg_capture_descs": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch), vp, C.POINTER(Capture),
                                        vp]),
        "xfg_capture_descs_frags": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch), vp,
                                              C.POINTER(Capture), C.c_uint32, vp]),
        "xfg_classify_timed": (C.c_int, [vp, C.c_int, C.POINTER(Batch), vp, C.c_int,
                                         C.POINTER(C.c_double)]),
        "xfg_classify_descs_timed": (C.c_int, [vp, C.c_int, C.POINTER(DescBatch), vp, C.c_int,
                                               C.POINTER(C.c_double)]),
        "xfg_stream_read_timed": (C.c_int, [vp, C.c_int, vp, C.c_uint64, C.c_int,
                                            C.POINTER(C.c_double)]),
        "xfg_stats_read": (C.c_int, [vp, C.POINTER(StatsRecord)]),
        "xfg_stats_read_dev": (C.c_int, [vp, C.c_int, C.POINTER(StatsRecord)]),
        "xfg_stats_reset": (C.c_int, [vp]),
        "xfg_sync": (C.c_int, [vp]),
        "xfg_dev_alloc": (vp, [vp, C.c_int, C.c_size_t]),
        "xfg_dev_free": (None, [vp, C.c_int, vp]),
        "xfg_memcpy_h2d": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t]),
        "xfg_memcpy_d2h": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t]),
        "xfg_host_alloc_pinned": (vp, [C.c_size_t]),
        "xfg_host_free_pinned": (None, [vp]),
        "xfg_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
        "xfg_comm_init": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
        "xfg_comm_allreduce": (C.c_int, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


lib = _load()


def _check(rc, what=""):
    if rc < 0:
        raise OSError(-rc, f"{what}: {lib.xfg_strerror(rc).decode()} ({rc})")
    return rc


def select_program(features: int):
    name = C.c_char_p()
    feats = C.c_uint32()
    _check(lib.xfg_select_program(features, C.byref(name), C.byref(feats)), "select_program")
    return name.value.decode(), feats.value


def read_pcap(path):
    """pcap / pcapng file -> (data u8, offsets u64, lens u32, orig_lens u32, ts_ns u64),
    frames at 16-byte aligned offsets (xfg_pcap_read)."""
    hb = HostBatch()
    _check(lib.xfg_pcap_read(os.fsencode(path), C.byref(hb)), "pcap_read")
    try:
        n = hb.count
        data = np.ctypeslib.as_array((C.c_uint8 * max(hb.bytes + 16, 16)).from_address(hb.data)).copy()
        out = [data]
        for ptr_, dt in ((hb.offsets, np.uint64), (hb.lens, np.uint32), (hb.orig_lens, np.uint32),
                         (hb.ts_ns, np.uint64)):
            out.append(np.ctypeslib.as_array(ptr_, shape=(n,)).astype(dt) if n else np.zeros(0, dt))
        return tuple(out)
    finally:
        lib.xfg_host_batch_free(C.byref(hb))


def _host_batch(data, offsets, lens, orig_lens, ts_ns):
    """struct xfg_host_batch over numpy arrays, and the arrays (kept alive by the caller);
    orig_lens / ts_ns None: the array is absent (NULL)."""
    data = np.ascontiguousarray(data, np.uint8)
    offs = np.ascontiguousarray(offsets, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint32)
    ol = None if orig_lens is None else np.ascontiguousarray(orig_lens, np.uint32)
    ts = None if ts_ns is None else np.ascontiguousarray(ts_ns, np.uint64)
    hb = HostBatch(data.ctypes.data, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                   lens.ctypes.data_as(C.POINTER(C.c_uint32)),
                   None if ol is None else ol.ctypes.data_as(C.POINTER(C.c_uint32)),
                   None if ts is None else ts.ctypes.data_as(C.POINTER(C.c_uint64)),
                   len(lens), data.nbytes, 1, 0)
    return hb, (data, offs, lens, ol, ts)


def pcapng_write_captured(path, ifname, data, offsets, lens, verdicts, action_mask, snaplen=0,
                          orig_lens=None, ts_ns=None):
    """pcapng capture of the frames whose verdict's bit is set in action_mask, cut to
    snaplen (xfg_pcapng_write_captured)."""
    hb, keep = _host_batch(data, offsets, lens, orig_lens, ts_ns)
    v = np.ascontiguousarray(verdicts, np.uint8)
    _check(lib.xfg_pcapng_write_captured(os.fsencode(path), None if ifname is None else
                                         ifname.encode(), C.byref(hb),
                                         v.ctypes.data_as(C.POINTER(C.c_uint8)), action_mask,
                                         snaplen), "pcapng_write_captured")
    del keep


def pcapng_begin(path, ifname, snaplen=0):
    """Create or truncate a capture file: its section and interface blocks (xfg_pcapng_begin)."""
    _check(lib.xfg_pcapng_begin(os.fsencode(path), None if ifname is None else ifname.encode(),
                                snaplen), "pcapng_begin")


def pcapng_append(path, blocks):
    """Append finished blocks, a capture call's output as it is (xfg_pcapng_append)."""
    b = blocks if isinstance(blocks, (bytes, bytearray)) else np.ascontiguousarray(blocks).tobytes()
    _check(lib.xfg_pcapng_append(os.fsencode(path), b, len(b)), "pcapng_append")


def write_verdicts_pcapng(path, ifname, data, offsets, lens, verdicts, orig_lens=None, ts_ns=None):
    """pcapng dump with the EPB verdict option (xfg_pcapng_write_verdicts)."""
    n = len(lens)
    data = np.ascontiguousarray(data, np.uint8)
    offs = np.ascontiguousarray(offsets, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint32)
    ol = np.ascontiguousarray(orig_lens if orig_lens is not None else lens, np.uint32)
    ts = np.ascontiguousarray(ts_ns if ts_ns is not None else np.zeros(n), np.uint64)
    v = np.ascontiguousarray(verdicts, np.uint8)
    hb = HostBatch(data.ctypes.data, offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                   lens.ctypes.data_as(C.POINTER(C.c_uint32)),
                   ol.ctypes.data_as(C.POINTER(C.c_uint32)),
                   ts.ctypes.data_as(C.POINTER(C.c_uint64)), n, data.nbytes, 1, 0)
    _check(lib.xfg_pcapng_write_verdicts(os.fsencode(path), ifname.encode(), C.byref(hb),
                                         v.ctypes.data_as(C.POINTER(C.c_uint8))), "pcapng_write")


def store_stats(state_dir):
    recs = (StatsRecord * ACTION_MAX)()
    _check(lib.xfg_store_stats_read(os.fsencode(state_dir), recs), "store_stats_read")
    return np.array([[r.packets, r.bytes] for r in recs], np.uint64)


def _key_buf(map_id, key) -> C.Array:
    kl = KEYLEN[map_id]
    if map_id == MAP_PORTS and isinstance(key, int):
        return (C.c_uint8 * 4).from_buffer_copy(int(key).to_bytes(4, "little"))
    b = bytes(key)
    if len(b) != kl:
        raise ValueError(f"key must be {kl} bytes")
    return (C.c_uint8 * kl).from_buffer_copy(b)


class DeviceBuffer:
    """hipMalloc'ed device memory owned through the C ABI."""

    def __init__(self, filt: "Filter", dev: int, nbytes: int):
        self.filt, self.dev, self.nbytes = filt, dev, nbytes
        self.ptr = lib.xfg_dev_alloc(filt.ctx, dev, nbytes)
        if not self.ptr:
            raise MemoryError(f"xfg_dev_alloc({nbytes}) failed")

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(lib.xfg_memcpy_h2d(self.filt.ctx, self.dev, self.ptr, arr.ctypes.data, arr.nbytes), "h2d")

    def download(self, arr: np.ndarray):
        assert arr.flags.c_contiguous and arr.nbytes <= self.nbytes
        _check(lib.xfg_memcpy_d2h(self.filt.ctx, self.dev, arr.ctypes.data, self.ptr, arr.nbytes), "d2h")
        return arr

    def free(self):
        if self.ptr:
            lib.xfg_dev_free(self.filt.ctx, self.dev, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Fib:
    """An immutable IPv4 forwarding table (xfg_fib_create): routes as
    fib_routes() takes them, next hops as fib_nexthops() takes them.  On a
    host-only context only the host copy is built (lookup() reads it); on a
    device context the tables are uploaded to device dev once, here."""

    def __init__(self, filt: "Filter", routes, nexthops, dev=0):
        r = routes if isinstance(routes, C.Array) else fib_routes(routes)
        h = nexthops if isinstance(nexthops, C.Array) else fib_nexthops(nexthops)
        self.filt, self.dev, self.ptr = filt, dev, None
        out = C.c_void_p()
        _check(lib.xfg_fib_create(filt.ctx, dev, r, len(routes), h, len(nexthops), C.byref(out)),
               "fib_create")
        self.ptr = out

    def lookup(self, dst):
        """The next hop of the longest match of dst (host order), or None."""
        nh = C.c_uint32()
        rc = lib.xfg_fib_lookup_host(self.ptr, int(dst), C.byref(nh))
        if rc == -2:   # -ENOENT
            return None
        _check(rc, "fib_lookup_host")
        return nh.value

    def free(self):
        if self.ptr and getattr(self.filt, "ctx", None):
            lib.xfg_fib_free(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Filter:
    """One xfg context: a selected xdpfilt_* program, its maps, and devices."""

    def __init__(self, features=FEAT_ALL | FEAT_DENY, devices=None, ndev=None,
                 ipv4_capacity=0, ipv6_capacity=0, eth_capacity=0, hash_seed=0, qt_min_keys=0,
                 window=0, descs_min_packets=0):
        opts = OpenOpts()
        opts.sz = C.sizeof(OpenOpts)
        opts.features = features
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            self._devs = arr
            opts.devices = arr
            opts.ndev = len(devices)
        else:
            opts.ndev = 1 if ndev is None else ndev
        opts.ipv4_capacity = ipv4_capacity
        opts.ipv6_capacity = ipv6_capacity
        opts.eth_capacity = eth_capacity
        opts.hash_seed = hash_seed
        opts.qt_min_keys = qt_min_keys
        opts.window = window
        opts.descs_min_packets = descs_min_packets
        ctx = C.c_void_p()
        _check(lib.xfg_open(C.byref(ctx), C.byref(opts)), "xfg_open")
        self.ctx = ctx
        self.ndev = lib.xfg_num_devices(ctx)
        self.prog_name = lib.xfg_prog_name(ctx).decode()
        self.prog_features = lib.xfg_prog_features(ctx)

    def close(self):
        if getattr(self, "ctx", None):
            lib.xfg_close(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def nvals(self):
        return max(self.ndev, 1)

    # -- maps ----------------------------------------------------------------
    def lookup(self, map_id, key):
        vals = (C.c_uint64 * self.nvals)()
        _check(lib.xfg_map_lookup(self.ctx, map_id, _key_buf(map_id, key), vals), "lookup")
        return list(vals)

    def update(self, map_id, key, vals):
        if isinstance(vals, int):
            vals = [vals] * self.nvals
        arr = (C.c_uint64 * self.nvals)(*vals)
        _check(lib.xfg_map_update(self.ctx, map_id, _key_buf(map_id, key), arr), "update")

    def delete(self, map_id, key):
        _check(lib.xfg_map_delete(self.ctx, map_id, _key_buf(map_id, key)), "delete")

    def keys(self, map_id):
        kl = KEYLEN[map_id]
        out, prev = [], None
        nxt = (C.c_uint8 * kl)()
        while True:
            rc = lib.xfg_map_get_next_key(self.ctx, map_id, prev, nxt)
            if rc == -errno.ENOENT:
                return out
            _check(rc, "get_next_key")
            out.append(bytes(nxt))
            prev = (C.c_uint8 * kl).from_buffer_copy(bytes(nxt))

    def count(self, map_id):
        return _check(lib.xfg_map_count(self.ctx, map_id), "count")

    def update_batch_percpu(self, map_id, keys: np.ndarray, vals: np.ndarray):
        """vals[n, nvals]: one value per device, as bpf_map_update_elem on a per-CPU map."""
        keys = np.ascontiguousarray(keys, np.uint8)
        vals = np.ascontiguousarray(vals, np.uint64)
        assert vals.ndim == 2 and vals.shape[1] == self.nvals
        _check(lib.xfg_map_update_batch_percpu(self.ctx, map_id, keys.ctypes.data,
                                               vals.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               len(vals)), "update_batch_percpu")

    def store_load(self, state_dir):
        _check(lib.xfg_store_load(self.ctx, os.fsencode(state_dir)), "store_load")

    def store_save(self, state_dir):
        _check(lib.xfg_store_save(self.ctx, os.fsencode(state_dir)), "store_save")

    def update_batch(self, map_id, keys: np.ndarray, vals: np.ndarray):
        keys = np.ascontiguousarray(keys, np.uint8)
        vals = np.ascontiguousarray(vals, np.uint64)
        _check(lib.xfg_map_update_batch(self.ctx, map_id, keys.ctypes.data,
                                        vals.ctypes.data_as(C.POINTER(C.c_uint64)), len(vals)),
               "update_batch")

    def load_rules(self, rules):
        """Load a tools.xftools.RuleSet (ports + hash maps) on every device."""
        r = rules.prepared()
        nz = np.nonzero(r.ports)[0]
        if len(nz):
            self.update_batch(MAP_PORTS, nz.astype("<u4").view(np.uint8), r.ports[nz])
        if len(r.v4_vals):
            self.update_batch(MAP_IPV4, r.v4_keys, r.v4_vals)
        if len(r.v6_vals):
            self.update_batch(MAP_IPV6, r.v6_keys, r.v6_vals)
        if len(r.eth_vals):
            self.update_batch(MAP_ETHERNET, r.eth_keys, r.eth_vals)

    def lookup_batch(self, map_id, keys: np.ndarray):
        """Per-device values of many keys: (vals[n, ndev], present[n])."""
        if map_id == MAP_PORTS:
            keys = np.ascontiguousarray(np.asarray(keys, dtype="<u4")).view(np.uint8)
        keys = np.ascontiguousarray(keys, np.uint8)
        n = len(keys) // KEYLEN[map_id] if keys.ndim == 1 else len(keys)
        vals = np.zeros((n, self.nvals), np.uint64)
        present = np.zeros(n, np.uint8)
        _check(lib.xfg_map_lookup_batch(self.ctx, map_id, keys.ctypes.data, n,
                                        vals.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        present.ctypes.data_as(C.POINTER(C.c_uint8))),
               "lookup_batch")
        return vals, present

    def values_of(self, map_id, keys: np.ndarray, dev=None):
        """Per-rule values in key order: one device's, or summed over devices
        the way the CLI sums per-CPU counters (flags from the first device)."""
        vals, _ = self.lookup_batch(map_id, keys)
        if dev is not None:
            return vals[:, dev].copy()
        hits = (vals >> np.uint64(6)).sum(axis=1, dtype=np.uint64)
        return (hits << np.uint64(6)) | (vals[:, 0] & np.uint64(63))

    # -- data path -------------------------------------------------------------
    def alloc(self, nbytes, dev=0) -> DeviceBuffer:
        return DeviceBuffer(self, dev, nbytes)

    def classify(self, data_ptr, lens_ptr, count, stride, verdicts_ptr, offsets_ptr=None,
                 lens_u16=False, dev=0, stream=None):
        b = Batch(data_ptr, offsets_ptr, lens_ptr, count, stride, int(lens_u16))
        _check(lib.xfg_classify(self.ctx, dev, C.byref(b), verdicts_ptr, stream), "classify")

    def classify_descs(self, umem_ptr, descs_ptr, count, verdicts_ptr, first=0, mask=0xffffffff,
                       dev=0, stream=None):
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        _check(lib.xfg_classify_descs(self.ctx, dev, C.byref(b), verdicts_ptr, stream),
               "classify_descs")

    def classify_descs_timed(self, umem_ptr, descs_ptr, count, verdicts_ptr, iters, first=0,
                             mask=0xffffffff, dev=0):
        """@iters launches of a descriptor batch; the average ms of one
        (xfg_classify_descs_timed)."""
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        ms = C.c_double()
        _check(lib.xfg_classify_descs_timed(self.ctx, dev, C.byref(b), verdicts_ptr, iters,
                                            C.byref(ms)), "classify_descs_timed")
        return ms.value

    def classify_descs_frags(self, umem_ptr, descs_ptr, count, verdicts_ptr, pkt_of_ptr=None,
                             first=0, mask=0xffffffff, dev=0, stream=None):
        """A descriptor batch whose packets may span several records
        (XDP_PKT_CONTD): one verdict byte per record of a complete packet,
        from its head record (xfg_classify_descs_frags).  Returns the counts
        (packets, records in them, records of the trailing incomplete one)."""
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        fr = Frags(C.sizeof(Frags), pkt_of_ptr)
        _check(lib.xfg_classify_descs_frags(self.ctx, dev, C.byref(b), C.byref(fr), verdicts_ptr,
                                            stream), "classify_descs_frags")
        return tuple(int(c) for c in fr.counts)

    def classify_descs_frags_timed(self, umem_ptr, descs_ptr, count, verdicts_ptr,
                                   pkt_of_ptr=None, first=0, mask=0xffffffff, dev=0):
        """One such call with its steps timed: (counts, (head pass ms,
        classify ms, spread ms)) (xfg_classify_descs_frags_timed)."""
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        fr = Frags(C.sizeof(Frags), pkt_of_ptr)
        ms = (C.c_double * 3)()
        _check(lib.xfg_classify_descs_frags_timed(self.ctx, dev, C.byref(b), C.byref(fr),
                                                  verdicts_ptr, ms), "classify_descs_frags_timed")
        return tuple(int(c) for c in fr.counts), tuple(ms)

    def classify_chain(self, data_ptr, lens_ptr, count, stride, verdicts_ptr,
                       chain_mask=CHAIN_PASS, idx_ptr=None, offsets_ptr=None, lens_u16=False,
                       dev=0, stream=None):
        """A chained stage over a batch (xfg_classify_chain): this context's
        program on the frames whose verdict byte (what an earlier stage wrote
        to verdicts_ptr) is in chain_mask; their bytes replaced, the others
        kept.  Returns the counts (selected, not selected)."""
        b = Batch(data_ptr, offsets_ptr, lens_ptr, count, stride, int(lens_u16))
        ch = Chain(C.sizeof(Chain), chain_mask, 0, idx_ptr)
        _check(lib.xfg_classify_chain(self.ctx, dev, C.byref(b), C.byref(ch), verdicts_ptr,
                                      stream), "classify_chain")
        return tuple(int(c) for c in ch.counts)

    def classify_descs_chain(self, umem_ptr, descs_ptr, count, verdicts_ptr,
                             chain_mask=CHAIN_PASS, idx_ptr=None, first=0, mask=0xffffffff,
                             dev=0, stream=None):
        """The same over a descriptor batch (xfg_classify_descs_chain).
        Returns the counts (selected, not selected)."""
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        ch = Chain(C.sizeof(Chain), chain_mask, 0, idx_ptr)
        _check(lib.xfg_classify_descs_chain(self.ctx, dev, C.byref(b), C.byref(ch), verdicts_ptr,
                                            stream), "classify_descs_chain")
        return tuple(int(c) for c in ch.counts)

    def classify_descs_chain_timed(self, umem_ptr, descs_ptr, count, verdicts_ptr,
                                   chain_mask=CHAIN_PASS, idx_ptr=None, first=0,
                                   mask=0xffffffff, dev=0):
        """One such call with its steps timed: (counts, (select pass ms,
        classify ms, scatter ms)) (xfg_classify_descs_chain_timed)."""
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        ch = Chain(C.sizeof(Chain), chain_mask, 0, idx_ptr)
        ms = (C.c_double * 3)()
        _check(lib.xfg_classify_descs_chain_timed(self.ctx, dev, C.byref(b), C.byref(ch),
                                                  verdicts_ptr, ms), "classify_descs_chain_timed")
        return tuple(int(c) for c in ch.counts), tuple(ms)

    def classify_descs_frags_chain(self, umem_ptr, descs_ptr, count, verdicts_ptr,
                                   chain_mask=CHAIN_PASS, idx_ptr=None, first=0,
                                   mask=0xffffffff, dev=0, stream=None):
        """A chained stage over a multi-buffer batch
        (xfg_classify_descs_frags_chain): this context's program on the
        complete packets whose head's byte at verdicts_ptr is in chain_mask,
        the new verdict on all their records.  Returns the counts (packets
        selected, records in them, all other records)."""
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        ch = FragsChain(C.sizeof(FragsChain), chain_mask, 0, idx_ptr)
        _check(lib.xfg_classify_descs_frags_chain(self.ctx, dev, C.byref(b), C.byref(ch),
                                                  verdicts_ptr, stream),
               "classify_descs_frags_chain")
        return tuple(int(c) for c in ch.counts)

    def classify_descs_frags_chain_timed(self, umem_ptr, descs_ptr, count, verdicts_ptr,
                                         chain_mask=CHAIN_PASS, idx_ptr=None, first=0,
                                         mask=0xffffffff, dev=0):
        """One such call with its steps timed: (counts, (pre-pass ms, classify
        ms, spread ms)) (xfg_classify_descs_frags_chain_timed)."""
        b = DescBatch(umem_ptr, descs_ptr, first, mask, count)
        ch = FragsChain(C.sizeof(FragsChain), chain_mask, 0, idx_ptr)
        ms = (C.c_double * 3)()
        _check(lib.xfg_classify_descs_frags_chain_timed(self.ctx, dev, C.byref(b), C.byref(ch),
                                                        verdicts_ptr, ms),
               "classify_descs_frags_chain_timed")
        return tuple(int(c) for c in ch.counts), tuple(ms)

    def host_register(self, arr: np.ndarray):
        """Pin and map a long-lived host array: the kernels read batches in it
        in place (xfg_host_register, zero copy)."""
        _check(lib.xfg_host_register(self.ctx, arr.ctypes.data, arr.nbytes), "host_register")

    def host_unregister(self, arr: np.ndarray):
        _check(lib.xfg_host_unregister(self.ctx, arr.ctypes.data), "host_unregister")

    def classify_xsk_host(self, umem: np.ndarray, descs: np.ndarray, count, first=0,
                          mask=0xffffffff, dev=0):
        """AF_XDP RX ring + UMEM in host memory (xfg_classify_xsk_host);
        descs: uint64 [entries, 2] xdp_desc records.  Returns verdicts."""
        verdicts = np.zeros(count, np.uint8)
        umem = np.ascontiguousarray(umem)
        descs = np.ascontiguousarray(descs, np.uint64)
        b = DescBatch(umem.ctypes.data, descs.ctypes.data, first, mask, count)
        _check(lib.xfg_classify_xsk_host(self.ctx, dev, C.byref(b), umem.nbytes,
                                         verdicts.ctypes.data), "classify_xsk_host")
        return verdicts

    def compact(self, verdicts_ptr, n, action, idx_ptr, count_ptr, dev=0, stream=None):
        _check(lib.xfg_compact(self.ctx, dev, verdicts_ptr, n, action, idx_ptr, count_ptr, stream),
               "compact")

    def ring_egress(self, rx_ptr, count, verdicts_ptr, counts_ptr, tx_ptr=None, fill_ptr=None,
                    rx_first=0, rx_mask=0xffffffff, tx_first=0, tx_mask=0xffffffff,
                    fill_first=0, fill_mask=0xffffffff, umem_ptr=None, flags=0, dev=0,
                    stream=None):
        """TX records of the PASS frames and fill addresses of the others from
        an RX descriptor batch and its verdicts (xfg_ring_egress); device
        pointers, counts_ptr: two u64 {TX records, fill addresses}."""
        e = Egress(C.sizeof(Egress), umem_ptr, rx_ptr, rx_first, rx_mask, tx_ptr, tx_first,
                   tx_mask, fill_ptr, fill_first, fill_mask, count, counts_ptr, flags)
        _check(lib.xfg_ring_egress(self.ctx, dev, C.byref(e), verdicts_ptr, stream),
               "ring_egress")

    def steer_egress(self, umem_ptr, rx_ptr, count, verdicts_ptr, counts_ptr, queues, avail=None,
                     mode=STEER_L4_HASH, skip_queue=0, nqueues=None, fill_ptr=None, rx_first=0,
                     rx_mask=0xffffffff, fill_first=0, fill_mask=0xffffffff, queue_of_ptr=None,
                     flags=0, dev=0, stream=None):
        """The PASS frames of an RX descriptor batch over the workers' TX rings
        by flow, the others' chunks to the fill ring (xfg_steer_egress).
        queues: a host table from steer_queues() (or what it takes); avail: the
        queue numbers the hash or port indexes (None: the identity); counts_ptr:
        nqueues + 2 u64 on the device.  Both tables may be overwritten as soon
        as this returns."""
        tab = queues if isinstance(queues, C.Array) else steer_queues(queues)
        av = None if avail is None else (C.c_uint32 * max(len(avail), 1))(*[int(a) for a in avail])
        s = Steer(C.sizeof(Steer), umem_ptr, rx_ptr, rx_first, rx_mask, tab, av,
                  len(queues) if nqueues is None else nqueues, 0 if avail is None else len(avail),
                  mode, skip_queue, fill_ptr, fill_first, fill_mask, count, counts_ptr,
                  queue_of_ptr, flags)
        _check(lib.xfg_steer_egress(self.ctx, dev, C.byref(s), verdicts_ptr, stream),
               "steer_egress")

    def steer_frags_egress(self, umem_ptr, rx_ptr, count, verdicts_ptr, counts_ptr, queues,
                           avail=None, mode=STEER_L4_HASH, skip_queue=0, nqueues=None,
                           fill_ptr=None, rx_first=0, rx_mask=0xffffffff, fill_first=0,
                           fill_mask=0xffffffff, queue_of_ptr=None, flags=0, dev=0, stream=None):
        """The same over multi-buffer packets (xfg_steer_frags_egress): every
        live record of a packet whose head is PASS to the TX ring of the head
        frame's queue, every live record of any other packet to the fill ring;
        a record whose verdict byte is VERDICT_NONE to neither.  Arguments as
        for steer_egress; flags may carry EGRESS_MULTIBUF."""
        tab = queues if isinstance(queues, C.Array) else steer_queues(queues)
        av = None if avail is None else (C.c_uint32 * max(len(avail), 1))(*[int(a) for a in avail])
        s = Steer(C.sizeof(Steer), umem_ptr, rx_ptr, rx_first, rx_mask, tab, av,
                  len(queues) if nqueues is None else nqueues, 0 if avail is None else len(avail),
                  mode, skip_queue, fill_ptr, fill_first, fill_mask, count, counts_ptr,
                  queue_of_ptr, flags)
        _check(lib.xfg_steer_frags_egress(self.ctx, dev, C.byref(s), verdicts_ptr, stream),
               "steer_frags_egress")

    def forward_egress(self, umem_ptr, rx_ptr, count, verdicts_ptr, counts_ptr, fib, ports, stack,
                       nports=None, fill_ptr=None, rx_first=0, rx_mask=0xffffffff, fill_first=0,
                       fill_mask=0xffffffff, queue_of_ptr=None, reason_of_ptr=None, flags=0,
                       dev=0, stream=None):
        """The PASS frames of an RX descriptor batch to the TX ring of the port
        a FIB lookup names, their TTL, checksum and MACs rewritten in the UMEM;
        the PASS frames that are not forwarded to the stack ring; the others'
        chunks to the fill ring (xfg_forward_egress).  fib: a Fib; ports: a host
        table from fwd_ports() (or what it takes); stack: a SteerQueue, a
        (tx_ptr, tx_first, tx_mask) triple or a bare pointer; counts_ptr:
        nports + 2 + FWD_REASONS u64 on the device.  The port table may be
        overwritten as soon as this returns."""
        tab = ports if isinstance(ports, C.Array) else fwd_ports(ports)
        f = Forward(C.sizeof(Forward), umem_ptr, rx_ptr, rx_first, rx_mask,
                    fib.ptr if isinstance(fib, Fib) else fib, tab,
                    len(ports) if nports is None else nports, steer_queues([stack])[0],
                    fill_ptr, fill_first, fill_mask, count, counts_ptr, queue_of_ptr,
                    reason_of_ptr, flags)
        _check(lib.xfg_forward_egress(self.ctx, dev, C.byref(f), verdicts_ptr, stream),
               "forward_egress")

    def forward_frags_egress(self, umem_ptr, rx_ptr, count, verdicts_ptr, counts_ptr, fib, ports,
                             stack, nports=None, fill_ptr=None, rx_first=0, rx_mask=0xffffffff,
                             fill_first=0, fill_mask=0xffffffff, queue_of_ptr=None,
                             reason_of_ptr=None, flags=0, dev=0, stream=None):
        """The same over multi-buffer packets (xfg_forward_frags_egress): every
        live record of a packet whose head is PASS to the TX ring the program
        gives the head buffer (a port's, the head rewritten, or the stack
        ring), every live record of any other packet to the fill ring; a record
        whose verdict byte is VERDICT_NONE to neither.  Arguments as for
        forward_egress; flags may carry EGRESS_MULTIBUF."""
        tab = ports if isinstance(ports, C.Array) else fwd_ports(ports)
        f = Forward(C.sizeof(Forward), umem_ptr, rx_ptr, rx_first, rx_mask,
                    fib.ptr if isinstance(fib, Fib) else fib, tab,
                    len(ports) if nports is None else nports, steer_queues([stack])[0],
                    fill_ptr, fill_first, fill_mask, count, counts_ptr, queue_of_ptr,
                    reason_of_ptr, flags)
        _check(lib.xfg_forward_frags_egress(self.ctx, dev, C.byref(f), verdicts_ptr, stream),
               "forward_frags_egress")

    def classify_socks(self, umem_ptr, socks, verdicts_ptr, nsocks=None, flat_ptr=None, dev=0,
                       stream=None):
        """One classify for the RX batches of many sockets over one UMEM
        (xfg_classify_socks).  socks: a host table from sock_table() (or what
        it takes); verdicts in flat order, socket after socket.  The table may
        be overwritten as soon as this returns."""
        tab = socks if isinstance(socks, C.Array) else sock_table(socks)
        sk = Socks(C.sizeof(Socks), umem_ptr, tab, flat_ptr, len(socks) if nsocks is None else nsocks)
        _check(lib.xfg_classify_socks(self.ctx, dev, C.byref(sk), verdicts_ptr, stream),
               "classify_socks")

    def socks_egress(self, socks, verdicts_ptr, counts_ptr, nsocks=None, fill_ptr=None,
                     fill_first=0, fill_mask=0xffffffff, umem_ptr=None, flags=0, dev=0,
                     stream=None):
        """Every socket's TX records, and the fill addresses into the shared
        ring at fill_ptr or (None) every socket's own, in one launch
        (xfg_socks_egress); counts_ptr: 2 * nsocks + 2 u64 on the device."""
        tab = socks if isinstance(socks, C.Array) else sock_table(socks)
        sk = Socks(C.sizeof(Socks), umem_ptr, tab, None, len(socks) if nsocks is None else nsocks)
        e = SocksEgress(C.sizeof(SocksEgress), fill_ptr, fill_first, fill_mask, counts_ptr, flags)
        _check(lib.xfg_socks_egress(self.ctx, dev, C.byref(sk), C.byref(e), verdicts_ptr, stream),
               "socks_egress")

    def classify_socks_frags(self, umem_ptr, socks, verdicts_ptr, nsocks=None, pkt_of_ptr=None,
                             flat_ptr=None, dev=0, stream=None):
        """One classify for the multi-buffer RX batches of many sockets over
        one UMEM (xfg_classify_socks_frags): a verdict byte per record in flat
        order, VERDICT_NONE for a socket's trailing incomplete packet.
        Returns (done, counts): done[s] the records of socket s in complete
        packets (u32 array), counts (packets, records in them, trailing)."""
        tab = socks if isinstance(socks, C.Array) else sock_table(socks)
        ns = len(socks) if nsocks is None else nsocks
        sk = Socks(C.sizeof(Socks), umem_ptr, tab, flat_ptr, ns)
        done = np.zeros(max(ns, 1), np.uint32)
        fr = SocksFrags(C.sizeof(SocksFrags), done.ctypes.data_as(C.POINTER(C.c_uint32)), pkt_of_ptr)
        _check(lib.xfg_classify_socks_frags(self.ctx, dev, C.byref(sk), C.byref(fr), verdicts_ptr,
                                            stream), "classify_socks_frags")
        return done[:ns], tuple(int(c) for c in fr.counts)

    def socks_frags_egress(self, socks, verdicts_ptr, counts_ptr, done=None, nsocks=None,
                           fill_ptr=None, fill_first=0, fill_mask=0xffffffff, umem_ptr=None,
                           flags=0, dev=0, stream=None):
        """xfg_socks_egress for multi-buffer batches (xfg_socks_frags_egress):
        done[s] records of socket s are live (None: all), a TX record keeps
        XDP_PKT_CONTD; counts_ptr: 2 * nsocks + 2 u64 on the device."""
        tab = socks if isinstance(socks, C.Array) else sock_table(socks)
        sk = Socks(C.sizeof(Socks), umem_ptr, tab, None, len(socks) if nsocks is None else nsocks)
        e = SocksEgress(C.sizeof(SocksEgress), fill_ptr, fill_first, fill_mask, counts_ptr, flags)
        d = None
        if done is not None:
            done = np.ascontiguousarray(done, np.uint32)
            d = done.ctypes.data_as(C.POINTER(C.c_uint32))
        _check(lib.xfg_socks_frags_egress(self.ctx, dev, C.byref(sk), C.byref(e), d, verdicts_ptr,
                                          stream), "socks_frags_egress")

    def capture_into(self, batch, verdicts_ptr, action_mask, out_ptr, out_bytes, counts_ptr,
                     snaplen=0, ts_ns_ptr=None, ts0=0, dev=0, stream=None):
        """The selected frames of a device batch (a Batch or a DescBatch of device pointers)
        as pcapng blocks at out_ptr (xfg_capture, xfg_capture_descs); counts_ptr: three u64
        {blocks written, their bytes, selected frames not written}.  Stream-ordered."""
        c = Capture(C.sizeof(Capture), action_mask, snaplen, ts_ns_ptr, ts0, out_ptr, out_bytes,
                    counts_ptr)
        if isinstance(batch, DescBatch):
            _check(lib.xfg_capture_descs(self.ctx, dev, C.byref(batch), verdicts_ptr, C.byref(c),
                                         stream), "capture_descs")
        else:
            _check(lib.xfg_capture(self.ctx, dev, C.byref(batch), verdicts_ptr, C.byref(c),
                                   stream), "capture")

    def capture(self, batch, verdicts, action_mask, snaplen=0, out_bytes=1 << 26, ts_ns=None,
                ts0=0, dev=0, stream=None):
        """capture_into() a buffer of out_bytes of its own, then only the counts and the
        written bytes come back: (blocks: uint8 array of counts[1] bytes, written, lost).
        batch: a Batch of device pointers; verdicts, ts_ns: device pointers."""
        room = (max(out_bytes, 16) + 15) & ~15
        d_out, d_c = self.alloc(room, dev), self.alloc(32, dev)
        try:
            self.capture_into(batch, verdicts, action_mask, d_out.ptr if out_bytes else None,
                              out_bytes, d_c.ptr, snaplen, ts_ns, ts0, dev, stream)
            self.sync()
            counts = d_c.download(np.zeros(3, np.uint64))
            blocks = d_out.download(np.zeros(int(counts[1]), np.uint8))
        finally:
            d_out.free()
            d_c.free()
        return blocks, int(counts[0]), int(counts[2])

    def capture_descs(self, batch, verdicts, action_mask, snaplen=0, out_bytes=1 << 26, ts_ns=None,
                      ts0=0, dev=0, stream=None):
        """capture() of an AF_XDP descriptor batch (a DescBatch of device pointers)."""
        assert isinstance(batch, DescBatch)
        return self.capture(batch, verdicts, action_mask, snaplen, out_bytes, ts_ns, ts0, dev,
                            stream)

    def capture_frags_into(self, batch, verdicts_ptr, action_mask, out_ptr, out_bytes, counts_ptr,
                           snaplen=0, ts_ns_ptr=None, ts0=0, flags=0, dev=0, stream=None):
        """capture_into() of a DescBatch of multi-buffer packets, one block a packet
        (xfg_capture_descs_frags); flags: CAPTURE_HEAD_ONLY.  Stream-ordered."""
        assert isinstance(batch, DescBatch)
        c = Capture(C.sizeof(Capture), action_mask, snaplen, ts_ns_ptr, ts0, out_ptr, out_bytes,
                    counts_ptr)
        _check(lib.xfg_capture_descs_frags(self.ctx, dev, C.byref(batch), verdicts_ptr,
                                           C.byref(c), flags, stream), "capture_descs_frags")

    def capture_descs_frags(self, batch, verdicts, action_mask, snaplen=0, out_bytes=1 << 26,
                            ts_ns=None, ts0=0, flags=0, dev=0, stream=None):
        """capture_frags_into() a buffer of out_bytes of its own: (blocks, written, lost) as
        capture_descs() returns them, over packets."""
        room = (max(out_bytes, 16) + 15) & ~15
        d_out, d_c = self.alloc(room, dev), self.alloc(32, dev)
        try:
            self.capture_frags_into(batch, verdicts, action_mask, d_out.ptr if out_bytes else None,
                                    out_bytes, d_c.ptr, snaplen, ts_ns, ts0, flags, dev, stream)
            self.sync()
            counts = d_c.download(np.zeros(3, np.uint64))
            blocks = d_out.download(np.zeros(int(counts[1]), np.uint8))
        finally:
            d_out.free()
            d_c.free()
        return blocks, int(counts[0]), int(counts[2])

    def classify_timed(self, data_ptr, lens_ptr, count, stride, verdicts_ptr, iters,
                       offsets_ptr=None, lens_u16=False, dev=0):
        b = Batch(data_ptr, offsets_ptr, lens_ptr, count, stride, int(lens_u16))
        ms = C.c_double()
        _check(lib.xfg_classify_timed(self.ctx, dev, C.byref(b), verdicts_ptr, iters,
                                      C.byref(ms)), "classify_timed")
        return ms.value

    def stream_read_timed(self, ptr, nbytes, iters, dev=0):
        ms = C.c_double()
        _check(lib.xfg_stream_read_timed(self.ctx, dev, ptr, nbytes, iters, C.byref(ms)),
               "stream_read_timed")
        return ms.value

    def classify_host(self, data: np.ndarray, lens: np.ndarray, stride=0, offsets=None, dev=0):
        """Host-resident batch (copies included); returns verdicts."""
        n = len(lens)
        verdicts = np.zeros(n, np.uint8)
        lens = np.ascontiguousarray(lens)
        offs = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
        b = Batch(data.ctypes.data, None if offs is None else offs.ctypes.data,
                  lens.ctypes.data, n, stride, int(lens.dtype == np.uint16))
        _check(lib.xfg_classify_host(self.ctx, dev, C.byref(b), verdicts.ctypes.data),
               "classify_host")
        return verdicts

    def run(self, data: np.ndarray, lens: np.ndarray, stride=0, offsets=None, dev=0):
        """Upload a host batch, classify it on the device, return verdicts
        (test convenience: device-resident classify + explicit copies)."""
        n = len(lens)
        lens = np.ascontiguousarray(lens)
        d_data = self.alloc(max(data.nbytes, 16) + 64, dev)
        d_data.upload(data)
        d_lens = self.alloc(max(lens.nbytes, 16), dev)
        d_lens.upload(lens)
        d_offs = None
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, np.uint64)
            d_offs = self.alloc(max(offsets.nbytes, 16), dev)
            d_offs.upload(offsets)
        d_v = self.alloc(max(n, 16), dev)
        self.classify(d_data.ptr, d_lens.ptr, n, stride, d_v.ptr,
                      offsets_ptr=None if d_offs is None else d_offs.ptr,
                      lens_u16=lens.dtype == np.uint16, dev=dev)
        self.sync()
        out = np.zeros(n, np.uint8)
        if n:
            d_v.download(out)
        for b in (d_data, d_lens, d_offs, d_v):
            if b is not None:
                b.free()
        return out

    def stats(self, dev=None) -> np.ndarray:
        recs = (StatsRecord * ACTION_MAX)()
        if dev is None:
            _check(lib.xfg_stats_read(self.ctx, recs), "stats_read")
        else:
            _check(lib.xfg_stats_read_dev(self.ctx, dev, recs), "stats_read_dev")
        return np.array([[r.packets, r.bytes] for r in recs], np.uint64)

    def stats_reset(self):
        _check(lib.xfg_stats_reset(self.ctx), "stats_reset")

    PATH_GENERAL, PATH_PIPELINE, PATH_IPV4, PATH_QT, PATH_ETH = 0, 1, 2, 5, 6

    def last_path(self, dev=0) -> int:
        """The classify kernel of the last launch on @dev (xfg_last_path)."""
        return _check(lib.xfg_last_path(self.ctx, dev), "last_path")

    def sync(self):
        _check(lib.xfg_sync(self.ctx), "sync")

    # -- multi-process -----------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(lib.xfg_comm_unique_id(buf), "comm_unique_id")
        return bytes(buf)

    def comm_init(self, nranks, rank, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _check(lib.xfg_comm_init(self.ctx, nranks, rank, buf), "comm_init")

    def comm_allreduce(self):
        _check(lib.xfg_comm_allreduce(self.ctx), "comm_allreduce")

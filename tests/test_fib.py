"""The forwarding table of xfg_forward_egress (xfg_fib_create,
xfg_fib_lookup_host; xdp-tools_amd/csrc/xfg_fib.c) on a host-only context: its
longest-prefix match against tests/fwdmodel.py's brute force, every refusal,
and the builder under ASAN + UBSAN in a stand-alone program (tests/fib_check.c)
-- nothing is loaded into Python under a sanitizer."""
import ctypes as C
import errno
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import fwdmodel as M
import xfgpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NESTED = [(0x0a000000, 8, 0), (0x0a010000, 16, 1), (0x0a010200, 24, 2), (0x0a010280, 25, 3),
          (0x0a0102c8, 32, 4)]                      # over 10.1.2.200
NNH = 300


@functools.lru_cache(maxsize=None)
def random_routes(seed, n=10000):
    """n distinct random routes with lengths 0..32 (a length has at most 2^len
    prefixes: the short ones come out fewer)."""
    rng = np.random.default_rng(seed)
    routes = {}
    while len(routes) < n:
        length = int(rng.integers(0, 33))
        prefix = int(rng.integers(1 << 32)) & M.mask_of(length)
        routes.setdefault((prefix, length), int(rng.integers(NNH)))
    return tuple((p, l, nh) for (p, l), nh in routes.items())


ROUTE_SETS = {"empty": (), "default": ((0, 0, 7),), "nested": tuple(NESTED),
              "random1": None, "random2": None, "random3": None}


def routes_of(name):
    return random_routes(int(name[-1])) if name.startswith("random") else ROUTE_SETS[name]


def nexthops(n=NNH):
    return [(1 + k, 0, 0, bytes(6), bytes(6)) for k in range(n)]


@pytest.fixture(scope="module")
def ctx():
    f = G.Filter(ndev=0)
    assert f.ndev == 0
    yield f
    f.close()


def lookup_all(fib, dsts):
    out = np.empty(len(dsts), np.int64)
    nh = C.c_uint32()
    for i, d in enumerate(dsts):
        rc = G.lib.xfg_fib_lookup_host(fib.ptr, int(d), C.byref(nh))
        assert rc in (0, -errno.ENOENT)
        out[i] = nh.value if rc == 0 else -1
    return out


@pytest.mark.parametrize("name", list(ROUTE_SETS))
def test_lookup_is_the_brute_force_lpm(ctx, name):
    routes = routes_of(name)
    rng = np.random.default_rng(len(routes))
    r = np.asarray(routes, np.int64).reshape(-1, 3)
    first = r[:, 0]
    last = first | np.array([~M.mask_of(int(l)) & 0xffffffff for l in r[:, 1]], np.int64)
    edges = np.concatenate([first, last, first - 1, last + 1]) & 0xffffffff
    inside = np.zeros(0, np.int64)
    if len(r):
        pick = rng.integers(0, len(r), 50000)
        inside = first[pick] | (rng.integers(0, 1 << 32, 50000) & (last - first)[pick])
    dsts = np.concatenate([edges, inside, rng.integers(0, 1 << 32, 100000 - len(inside)),
                           [0, 0xffffffff]]).astype(np.uint64)
    assert len(dsts) >= 100000
    fib = G.Fib(ctx, routes, nexthops())
    try:
        got = lookup_all(fib, dsts)
    finally:
        fib.free()
    np.testing.assert_array_equal(got, M.lpm_many(routes, dsts))
    # lpm_many is held to the route-by-route lpm() here too, on a sample
    for d in dsts[:: max(1, len(dsts) // 300)]:
        want = M.lpm(routes, int(d))
        assert M.lpm_many(routes, [d])[0] == (-1 if want is None else want)


def create(ctx, routes, nhs, nroutes=None, nnh=None, out=True, null_routes=False, null_nh=False):
    r, h = G.fib_routes(routes), G.fib_nexthops(nhs)
    o = C.c_void_p()
    rc = G.lib.xfg_fib_create(ctx, 0, None if null_routes else r, len(routes) if nroutes is None else nroutes,
                              None if null_nh else h, len(nhs) if nnh is None else nnh,
                              C.byref(o) if out else None)
    if rc == 0:
        G.lib.xfg_fib_free(o)
    return rc


def test_refusals(ctx):
    nh = nexthops(4)
    good = [(0x0a000000, 8, 0)]
    assert create(ctx.ctx, good, nh) == 0
    assert create(None, good, nh) == -errno.EINVAL
    assert create(ctx.ctx, good, nh, out=False) == -errno.EINVAL
    assert create(ctx.ctx, good, nh, null_routes=True) == -errno.EINVAL
    assert create(ctx.ctx, good, nh, null_nh=True) == -errno.EINVAL
    assert create(ctx.ctx, [(0, 33, 0)], nh) == -errno.EINVAL                 # len > 32
    assert create(ctx.ctx, [(0x0a000001, 8, 0)], nh) == -errno.EINVAL         # bits below len
    assert create(ctx.ctx, [(1, 0, 0)], nh) == -errno.EINVAL
    assert create(ctx.ctx, [(0x0a000001, 32, 0)], nh) == 0
    assert create(ctx.ctx, [(0x0a000000, 8, 4)], nh) == -errno.EINVAL         # nexthop >= nnexthops
    assert create(ctx.ctx, good, [(0, 0, 0, bytes(6), bytes(6))]) == -errno.EINVAL   # ifindex 0
    assert create(ctx.ctx, good + [(0x0b000000, 8, 1)] + good, nh) == -errno.EEXIST
    assert create(ctx.ctx, [(0, 0, 0), (0, 0, 1)], nh) == -errno.EEXIST
    assert create(ctx.ctx, [(0x0a000000, 8, 0), (0x0a000000, 9, 0)], nh) == 0  # same prefix, other len
    # the empty table, with and without arrays
    assert create(ctx.ctx, [], [], null_routes=True, null_nh=True) == 0
    assert G.lib.xfg_fib_lookup_host(None, 0, C.byref(C.c_uint32())) == -errno.EINVAL
    G.lib.xfg_fib_free(None)


def test_what_the_entry_format_holds(ctx):
    assert create(ctx.ctx, [(0, 0, G.FIB_NEXTHOPS_MAX - 1)], nexthops(G.FIB_NEXTHOPS_MAX)) == 0
    assert create(ctx.ctx, [(0, 0, 0)], nexthops(G.FIB_NEXTHOPS_MAX + 1)) == -errno.ENOSPC
    groups = [((k << 8) | 0x80, 25, 0) for k in range(G.FIB_GROUPS_MAX + 1)]
    assert create(ctx.ctx, groups[:-1], nexthops(1)) == 0
    assert create(ctx.ctx, groups, nexthops(1)) == -errno.ENOSPC
    # the last next hop and the last group answer
    fib = G.Fib(ctx, groups[:-1] + [(0, 0, G.FIB_NEXTHOPS_MAX - 1)], nexthops(G.FIB_NEXTHOPS_MAX))
    try:
        assert fib.lookup(((G.FIB_GROUPS_MAX - 1) << 8) | 0x81) == 0
        assert fib.lookup(((G.FIB_GROUPS_MAX - 1) << 8) | 0x7f) == G.FIB_NEXTHOPS_MAX - 1
    finally:
        fib.free()


def test_the_header_s_structures(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "xdpfilter_gpu.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(struct xfg_fib_nexthop),'
                   ' offsetof(struct xfg_fib_nexthop, mtu), offsetof(struct xfg_fib_nexthop, ret),'
                   ' offsetof(struct xfg_fib_nexthop, dmac), offsetof(struct xfg_fib_nexthop, smac),'
                   ' sizeof(struct xfg_fib_route), offsetof(struct xfg_fib_route, len),'
                   ' XFG_FIB_NEXTHOPS_MAX, XFG_FIB_GROUPS_MAX);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    N, R = G.FibNexthop, G.FibRoute
    assert got == [C.sizeof(N), N.mtu.offset, N.ret.offset, N.dmac.offset, N.smac.offset, C.sizeof(R),
                   R.len.offset, G.FIB_NEXTHOPS_MAX, G.FIB_GROUPS_MAX]


# ---- the builder under ASAN + UBSAN, in a program of its own
@pytest.fixture(scope="module")
def fib_check(tmp_path_factory):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    d = tmp_path_factory.mktemp("fib_check")
    probe = d / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run([cc, *san, "-o", str(d / "probe"), str(probe)], capture_output=True).returncode or \
            subprocess.run([str(d / "probe")], capture_output=True).returncode:
        pytest.skip("the C compiler has no ASAN/UBSAN runtime")
    exe = d / "fib_check"
    csrc = os.path.join(ROOT, "xdp-tools_amd", "csrc")
    subprocess.run([cc, "-O1", "-g", "-Wall", "-Wextra", "-std=gnu11", *san, "-I", os.path.join(ROOT, "include"),
                    "-I", csrc, "-o", str(exe), os.path.join(ROOT, "tests", "fib_check.c"),
                    os.path.join(csrc, "xfg_fib.c")], check=True)
    return exe, d


@pytest.mark.parametrize("name", list(ROUTE_SETS))
def test_builder_under_sanitizers(fib_check, name):
    exe, d = fib_check
    routes = routes_of(name)
    path = d / f"{name}.txt"
    path.write_text(f"{len(routes)} {NNH}\n" + "".join(f"{p:x} {l} {nh}\n" for p, l, nh in routes))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) >= 20000 + 4 * len(routes)

"""The classify launch plan (xdp-tools_amd/csrc/xfg_plan.c) on the CPU.

tests/golden/plan_cases.txt holds one line a launch, recorded on an MI355X
from the runtime as it was before the plan became a function of its own
(two passes in xfg_ctx.c, fill_kargs_src and launch_batch): the inputs the
decision read, " | ", and every field it decided.  tools/plan_replay (built
by `make`, tests/plan_replay.c) runs xfg_plan() over the inputs; every
recorded field must come out equal -- integers, no tolerance.

The hand-written cases are launches no test can make (2^32 packets) or
shapes the recording device does not have; each expectation is derived from
the rule as that earlier code stated it, quoted beside it.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "tools", "plan_replay")
CASES = os.path.join(ROOT, "tests", "golden", "plan_cases.txt")


def fields(text):
    return dict(t.split("=", 1) for t in text.split())


def replay(lines):
    out = subprocess.run([REPLAY], input="".join(l + "\n" for l in lines), text=True,
                         capture_output=True, check=True).stdout
    return {f["id"]: f for f in map(fields, out.splitlines())}


@pytest.fixture(scope="module")
def recorded():
    with open(CASES) as f:
        lines = f.read().splitlines()
    want = {}
    for l in lines:
        if l.startswith("case "):
            ins, outs = l[5:].split(" | ")
            want[fields(ins)["id"]] = fields(outs)
    return lines, want, replay(lines)


def test_matrix_complete(recorded):
    _, want, got = recorded
    assert sorted(want, key=int) == [str(i) for i in range(1, 41)]
    assert set(got) == set(want)


@pytest.mark.parametrize("case", range(1, 41))
def test_recorded_plan(recorded, case):
    _, want, got = recorded
    w, g = want[str(case)], got[str(case)]
    assert {k: g[k] for k in w} == w


def test_recorded_decisions(recorded):
    """The rows pin the decisions they were recorded for (ISSUE matrix)."""
    lines, want, _ = recorded
    kind = {i: int(want[str(i)]["kind"]) for i in range(1, 41)}
    assert [kind[i] for i in range(1, 27)] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 6, 6] + [5] * 11 + [0]
    assert [kind[i] for i in range(27, 41)] == [0, 1, 3, 2, 5, 5, 2, 5, 5, 1, 1, 5, 5, 5]
    w = lambda i, k: int(want[str(i)][k])  # noqa: E731
    assert w(6, "window") == 128 and w(5, "window") == 64
    assert w(7, "ek") and w(7, "bl_lds") and not w(8, "ek") and not w(9, "bl_lds")
    assert not w(10, "logs") and not w(11, "logs") and w(12, "logs")
    assert not w(15, "logs") and w(16, "logs") and w(16, "K") == 4
    # (row 17, 2^20 packets on 2^21 QT slots, logs only for the count wave: where the kernel
    # can launch with its histogram -- on the recording device it cannot, the occupancy
    # table's kind 7 is all 0, so the hand-written cases below cover the count wave)
    occ = fields(lines[0][4:])["occ"].split(",")
    cw = int(int(occ[7 * 32]) > 0)
    assert (w(17, "logs"), w(17, "cw"), w(17, "K")) == (cw, cw, 2 if cw else 1)
    assert w(18, "qt_dyn") and not w(17, "qt_dyn")
    assert (w(21, "v6d"), w(21, "v6p"), w(22, "v6p")) == (1, 1, 2)
    assert w(23, "ek") and w(23, "logs") and not w(23, "cw")
    assert w(24, "window") == 64 and w(25, "window") == 128 and not w(25, "cw")
    assert not w(32, "logs") and not w(34, "cw") and w(35, "K") == 1 and not w(36, "ek")
    assert not w(37, "bl_lds") and (w(38, "v6d"), w(38, "v6p")) == (1, 0) and w(39, "defer_sep")


# A device for the hand-written cases: 256 CUs; 512 threads a workgroup but
# the general kernel's 256; @occ workgroups a CU for every kernel.
def dev(occ, cw=1):
    o = [occ] * (9 * 32)
    o[7 * 32:8 * 32] = [cw] * 32
    return ("dev feat=95 ncu=256 thr=256,256," + ",".join(["512"] * 16) + " occ=" + ",".join(map(str, o)))


# C3-like: xdpfilt_dny_all, 20000 dst rules, nothing else; the quotient index
# of 2^17 buckets (2^21 slots) when asked for.
BASE = ("feat=95 offs=0 al16=1 descs=0 hwin=0 c4=20000 f4=2 b4=24576 s4=109236 c6=0 f6=0 b6=3750 "
        "s6=22224 ce=0 fe=0 be=3750 se=18186 fd4=0 ports=8 ptab=1 win=64 dmin=65536 ekok=0 "
        "qt_n=2097152 qt_live=2 qt_nimg=1 qt_bits=17 ek_slots=0")


def hand(occ, cid, n, stride, qtmin=1 << 18, cw=1):
    r = replay([dev(occ, cw), f"case id={cid} n={n} stride={stride} qtmin={qtmin} {BASE}"])[cid]
    return {k: int(v) for k, v in r.items() if k != "id" and "," not in v}


def test_packet_count_and_stride_bounds():
    # "a->pipe = !b->offsets && b->stride >= a->window && !(b->stride & 15) &&
    #  !((uintptr_t)b->data & 15) && b->count < (1ull << 32) && b->stride < 65536;"
    assert hand(2, "a", (1 << 32) - 1, 64)["kind"] == 2
    r = hand(2, "b", 1 << 32, 64)
    assert (r["kind"], r["pipe"], r["dense"]) == (0, 0, 0)
    assert hand(2, "c", 1 << 14, 65536 - 16)["kind"] == 2
    assert hand(2, "d", 1 << 14, 65536)["kind"] == 0


def test_byte_sum_bound():
    # "if (!db && a->pipe && (uint64_t)a->stride * (((b->count + 63) / 64 + 1023) / 1024 + 1)
    #      >= (1ull << 32)) a->pipe = 0;"
    # No batch the two limits above let through reaches it: the largest, stride 65520 (strides
    # are multiples of 16) and 2^32 - 1 packets, sums 65520 * 65537 < 2^32 and stays pipelined;
    # the first batch of that stride past the bound, of 65551 * 65536 + 1 packets, is the
    # general kernel's by the packet limit already.
    bound = lambda stride, n: stride * ((((n + 63) // 64 + 1023) // 1024) + 1)  # noqa: E731
    stride, n = 65520, (1 << 32) - 1
    assert bound(stride, n) == 65520 * 65537 < 1 << 32
    assert hand(2, "a", n, stride)["kind"] == 2
    n = 65551 * 65536 + 1
    assert bound(stride, n - 1) < 1 << 32 <= bound(stride, n) and n > 1 << 32
    assert hand(2, "b", n, stride)["kind"] == 0


def test_grid_of_one_packet():
    # "uint64_t need = (a.n + per_wg - 1) / per_wg; if (grid > need) grid = need ? need : 1;"
    assert hand(2, "a", 1, 64)["grid"] == 1
    assert hand(2, "b", 512 + 1, 64)["grid"] == 2


def test_pending_logs_shrink_to_the_slices():
    # "K = XFG_LOG_PEND_MAX; while (K > 1 && K * grid > XFG_LOG_SLICES_MAX) K--;" (1024 slices)
    n = 1 << 25   # (not below XFG_CW_MAX_PACKETS: no count wave)
    for occ, grid, k in ((1, 256, 4), (2, 512, 2), (3, 768, 1), (4, 1024, 1)):
        r = hand(occ, "a", n, 64, qtmin=1)
        assert (r["kind"], r["logs"], r["cw"], r["grid"], r["K"]) == (5, 1, 0, grid, k)
        assert r["pfill_bytes"] == 256 * k * grid * 4
    # "logs = ... && grid <= XFG_LOG_SLICES_MAX"
    r = hand(5, "b", n, 64, qtmin=1)
    assert (r["kind"], r["grid"], r["logs"], r["K"]) == (5, 1280, 0, 1)


def test_count_wave_needs_two_slice_sets():
    # "int cw = logs && a.qt && !pwide && hist <= XFG_CW_HIST_MAX && a.window <= 64 && !a.v6p &&
    #  !a.ek && 2 * grid <= XFG_LOG_SLICES_MAX && d->occ[7][0][occ_c] > 0 && a.n < XFG_CW_MAX_PACKETS;"
    n = 1 << 23
    r = hand(2, "a", n, 64, qtmin=1)
    assert (r["grid"], r["logs"], r["cw"], r["K"]) == (512, 1, 1, 2)
    r = hand(3, "b", n, 64, qtmin=1)
    assert (r["grid"], r["logs"], r["cw"], r["K"]) == (768, 1, 0, 1)
    # ... and a kernel that can launch with its histogram
    r = hand(2, "c", n, 64, qtmin=1, cw=0)
    assert (r["logs"], r["cw"], r["K"]) == (1, 0, 2)
    # "(2 * (uint64_t)d->qt_n > a.n && !(cw_cap && a.n >= cw_min))": below twice the QT slots
    # only the count wave's log runs
    assert hand(2, "d", 1 << 20, 64, qtmin=1)["logs"] == 1
    assert hand(3, "e", 1 << 20, 64, qtmin=1)["logs"] == 0

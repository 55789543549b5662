#!/usr/bin/env python3
"""tools/bench_configs.py — the BASELINE.json configurations beside C3
(SURVEY.md §8d), one GPU, one JSON line each:

  c2  xdpfilt_dny_ip, 1k IPv4 dst rules, 64 B frames, device-resident
  c4  xdpfilt_dny_all, IMIX 64/570/1514 (7:4:1), 1M IPv4 rules: one GPU's
      shard of the 8-GPU configuration (weak scaling: per-GPU work fixed)
  c5  xdpfilt_dny_all, 1514 B frames, 15M IPv4 + 1M IPv6 dst rules + 1024
      dst-port rules: device-resident, and end to end from host memory
      (header windows H2D, verdicts D2H, xfg_classify_host)
  c3  C3 itself at SURVEY.md §8d's 2^24 batch (bench.py times 2^26)
  c3sd  C3 with every rule src|dst (`-m src,dst`): both IPv4 lookups live,
      so a packet probes two keys (the case C3's all-dst census skips)
  c3e  C3 plus C1's 8 MAC rules (4 dst, 4 src; a ruled MAC in 10 % of the
      frames): Ethernet rules beside IP rules, the generic pipelined kernel
      with the Ethernet map as its LDS key table
  c3d  C3's workload as an AF_XDP descriptor batch (xfg_classify_descs_timed):
      the 64 B frames in a UMEM of 2 KiB chunks at headroom 256, chunks in
      random order, read through an RX ring that wraps.  With the diagnostics
      library (XFG_LIB=diag) also the same batch on the general kernel
      (XFG_KERNEL=general: what a descriptor batch ran before the pipelined
      descriptor mode) and, strided, on the generic pipelined kernel
      (XFG_KERNEL=generic) and the quotient-index kernel.  2^22 packets by
      default: an 8 GiB UMEM (the workload's 2^24 would need 32 GiB)
  c3f  c3d's batch classified, then its egress (xfg_ring_egress): TX records of
      the PASS frames and fill addresses of the others, with and without the
      MAC swap, beside xfg_compact on the same verdicts -- each timed over
      --iters launches between events on a caller stream, with the bytes
      moved and their share of this device's streaming-read rate
  c3st c3f's batch classified, then steered (xfg_steer_egress): the PASS
      frames over 1, 8 and 64 workers' TX rings in modes L4_HASH and L4_DPORT,
      beside xfg_ring_egress on the same batch and verdicts, timed as c3f's
      legs are; the records a queue gets (least, most) and the refused frames
  c3fw c3d's batch classified, then forwarded over 8 ports (xfg_forward_egress)
      by a FIB of 2^20 synthetic routes (80% /24, 20% /25../32, over a default
      route) and again by a FIB of the default route alone -- the difference is
      what the table costs -- beside xfg_steer_egress at K = 8 (L4_HASH) and
      xfg_ring_egress with the MAC swap on the same verdicts, timed as c3f's
      legs are; the PASS frames by reason after the first call, and the
      forwarded frames after every run (every call decrements their TTL: a run
      after which fewer frames are forwarded is left out of the figures)
  c3c  c3d's batch classified, then its DROP frames captured as pcapng blocks
      (xfg_capture_descs, snaplen 0), beside xfg_compact; the same ring with
      1514-byte frames at snaplen 96, one in ten selected; one tile of
      packets for the fixed cost of a call -- timed as c3f's legs are
  c3ch c3d's batch as the second stage of a chain (xfg_classify_descs_chain):
      the verdict bytes pre-set so that half the frames are selected, once
      every other frame and once a contiguous half.  The call by wall clock (to
      its return and to the stream's end) and its three steps
      (xfg_classify_descs_chain_timed); beside them xfg_classify_descs over a
      pre-built plain array of the same selected half (stage 2 alone: the
      floor), over the whole batch, and xfg_compact over the same verdict
      bytes, with the bytes the select pass and the compaction move
  c3m  c3d's UMEM and rules with every C3 frame the head of a 3-record packet
      (XDP_PKT_CONTD, a socket bound with XDP_USE_SG): two continuation chunks a
      packet, each holding a frame that hits a rule -- 2^22 packets, 3 * 2^22
      records.  xfg_classify_descs_frags: its head pass, the classify of the
      heads and the spread (events around each, xfg_classify_descs_frags_timed),
      the whole call (wall clock to its return, and to the stream's end), the
      egress with XFG_EGRESS_MULTIBUF timed as c3f's legs are, and c3d
      (xfg_classify_descs_timed) on the same heads for comparison
  c3mc c3m's batch classified by xfg_classify_descs_frags, then its DROP packets
      captured whole as pcapng blocks (xfg_capture_descs_frags, snaplen 0), and
      head only; beside them xfg_capture_descs over the same records and
      verdicts (the same payload bytes, three times the blocks) -- timed as
      c3c's legs are, with the bytes moved and their share of the
      streaming-read rate
  c3mst c3m's batch classified by xfg_classify_descs_frags, then steered by whole
      packets (xfg_steer_frags_egress): every record of a PASS packet to the TX
      ring of its head's queue, over 1, 8 and 64 rings in modes L4_HASH and
      L4_DPORT, beside xfg_ring_egress with XFG_EGRESS_MULTIBUF on the same
      records and verdicts; and the same records as single-record packets
      through xfg_steer_egress and xfg_steer_frags_egress (8 rings) -- timed as
      c3st's legs are
  c3mfw c3m's batch classified by xfg_classify_descs_frags, then forwarded by
      whole packets (xfg_forward_frags_egress) over 8 ports by c3fw's two FIBs,
      beside xfg_ring_egress with XFG_EGRESS_MULTIBUF on the same records and
      verdicts; and the same records as single-record packets through
      xfg_forward_egress and xfg_forward_frags_egress -- timed as c3fw's legs
      are, with its rule for the runs after which fewer packets are forwarded
  c3mch c3m's batch, classified by xfg_classify_descs_frags, as the first stage
      of a chain (xfg_classify_descs_frags_chain): half the packets' verdict
      bytes pre-set to PASS, once every other packet and once a contiguous
      half.  The call by wall clock (to its return and to the stream's end) and
      its three steps (xfg_classify_descs_frags_chain_timed); beside them the
      three steps of xfg_classify_descs_frags over a pre-built ring of the
      selected packets alone (the floor), with the bytes the pre-pass and the
      spread move
  c3s  C3's rules and frames in c3d's UMEM, scattered over --socks sockets of
      --batch records (64 x 64 by default; --sweep: 4, 64, 1024 sockets x 64,
      256 records): a poll round as xfg_classify_descs + xfg_ring_egress a
      socket beside one xfg_classify_socks + one xfg_socks_egress, whole rounds
      by host wall clock (the cost at issue is the calls' own), us a round,
      Mpps and the ratio
  c3sm  c3m's three-record packets scattered over --socks sockets of --batch
      records (same defaults and --sweep as c3s), odd sockets' batches ending in
      the middle of a packet: a poll round as xfg_classify_descs_frags +
      xfg_ring_egress(MULTIBUF) a socket beside one xfg_classify_socks_frags +
      one xfg_socks_frags_egress, first checked to produce the same rings; whole
      rounds by host wall clock (at least five runs a leg), each leg's classify
      and egress calls alone, and the ratio

  c1xdpfilt_alw_eth, the 8 MAC rules 02:00:00:00:00:0{1..8} (4 dst, 4
      src), 64 B Ethernet/IPv4/UDP frames, 25% carrying a ruled MAC (SURVEY.md
      §8d: BASELINE.json configs[0], the reference's in-kernel CPU case): the
      GPU path, and the CPU restatement timed on the same batch on 1 thread
      and on every usable host core (SURVEY §8d CPU item 2; the in-kernel
      veth run itself needs a BPF toolchain this image lacks)

Roofline bytes per packet are min(len, 128) + 1.
Usage: python3 tools/bench_configs.py [c2] [c4] [c5] [--log2-packets N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "xdp-tools_amd", "python"))

HBM_PEAK_GBS = 8000.0


def run_c1(args):
    import numpy as np
    import xftools as X
    import xfgpu as G
    sys.path.insert(0, ROOT)
    import bench
    n = 1 << (args.log2_packets or 24)
    rules = X.c1_rules()
    data, lens = X.gen_c1(1, n)
    f = G.Filter(X.VARIANT_FEATURES["xdpfilt_alw_eth"], devices=[0])
    assert f.prog_name == "xdpfilt_alw_eth"
    f.load_rules(rules)
    alg = int(np.minimum(lens.astype(np.int64), 128).sum() + n)
    d_data, d_lens, d_verd = f.alloc(data.nbytes), f.alloc(lens.nbytes), f.alloc(n)
    d_data.upload(data)
    d_lens.upload(lens)
    f.classify_timed(d_data.ptr, d_lens.ptr, n, 64, d_verd.ptr, 2)
    ms = f.classify_timed(d_data.ptr, d_lens.ptr, n, 64, d_verd.ptr, args.iters)
    path = f.last_path()
    f.close()
    if args.no_cpu:
        print(json.dumps({"config": "c1", "packets": n, "kernel_path": path,
                          "kernel_ms": round(ms, 4), "Mpps": round(n / (ms * 1e-3) / 1e6, 1),
                          "roofline": {"frac": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}),
              flush=True)
        return
    # the CPU restatement on the same batch: 1 thread and every usable core
    # (a bounded sample: whole passes until ~4 s each)
    feats = X.VARIANT_FEATURES["xdpfilt_alw_eth"]
    m = min(n, 1 << 22)
    prepared = rules.prepared()
    maps = X.OracleMaps(prepared, hashed=True)

    def rate(threads, secs=4.0):
        done, t0 = 0, time.perf_counter()
        while True:
            X.run_oracle(feats, data[:m * 64], lens[:m], prepared, stride=64, maps=maps,
                         nthreads=threads)
            done += m
            el = time.perf_counter() - t0
            if el >= secs:
                return done / el / 1e6
    nt = bench.host_threads()
    r1, rn = rate(1), rate(nt)
    line = {"config": "c1", "program": "xdpfilt_alw_eth", "packets": n, "stride": 64,
            "rules_eth": 8, "kernel_path": path, "kernel_ms": round(ms, 4),
            "Mpps": round(n / (ms * 1e-3) / 1e6, 1),
            "roofline": {"alg_bytes_per_launch": alg,
                         "achieved_GBps": round(alg / (ms * 1e-3) / 1e9, 1),
                         "frac": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "cpu_restatement": {"Mpps_1thread": round(r1, 2), "Mpps_all": round(rn, 2),
                                "threads": nt, "cpu_model": bench.cpu_model(),
                                "sample": f"2^{m.bit_length() - 1} packets of the same batch, "
                                          "whole passes for ~4 s each"},
            "in_kernel_xdp": "not measured: needs a BPF-capable clang, libbpf, bpffs, "
                             "iproute2 and root, absent from this image"}
    print(json.dumps(line), flush=True)


C3D_CHUNK, C3D_HEADROOM = 2048, 256


def c3d_workload(args, tag, umem_chunks=1, log2_default=22, descs_min_packets=1):
    """C3's frames in a device UMEM behind an RX ring that wraps, the rules
    loaded (c3d, c3f).  Returns a namespace of what the legs use.
    umem_chunks: the UMEM's chunks per frame (c3m's continuation chunks lie
    past the frames')."""
    import types
    import numpy as np
    import xftools as X
    import xfgpu as G
    n = 1 << (args.log2_packets or log2_default)
    n4, nports, stride = 1_000_000, 16, 64
    t0 = time.time()
    v4 = X.rand_keys(3, int(n4 * 1.02) + 16, 4)[:n4]
    ports = (np.arange(nports, dtype=np.uint32) * 61 + 53).astype(np.uint16)
    data, lens = X.gen_workload(3, 3, n, stride, v4=v4, ports=ports)
    # (descs_min_packets=1: the pipelined descriptor mode at any --log2-packets,
    # also below the size from which xfg_classify_descs takes it by default)
    f = G.Filter(G.FEAT_ALL | G.FEAT_DENY, devices=[0], ipv4_capacity=n4, ipv6_capacity=1024,
                 descs_min_packets=descs_min_packets)
    f.update_batch(G.MAP_IPV4, v4, np.full(len(v4), 2, np.uint64))
    pk = np.array([X.port_key(int(p)) for p in ports], "<u4").view(np.uint8)
    f.update_batch(G.MAP_PORTS, pk, np.full(len(ports), 2 | 4 | 8, np.uint64))
    # frame i in chunk perm[i]; the UMEM is built and uploaded a piece at a
    # time (chunk c holds frame inv[c])
    rng = np.random.default_rng(12)
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    d_umem = f.alloc(umem_chunks * n * C3D_CHUNK)
    frames = data.reshape(n, stride)
    piece = 1 << 17
    buf = np.zeros((piece, C3D_CHUNK), np.uint8)
    for c0 in range(0, n, piece):
        c1 = min(n, c0 + piece)
        buf[:c1 - c0, C3D_HEADROOM:C3D_HEADROOM + stride] = frames[inv[c0:c1]]
        G._check(G.lib.xfg_memcpy_h2d(f.ctx, 0, d_umem.ptr + c0 * C3D_CHUNK, buf.ctypes.data,
                                      (c1 - c0) * C3D_CHUNK), "memcpy_h2d")
    # the RX ring: twice the batch, the batch starting 777 before its end
    entries = 2 * n
    first = entries - 777
    descs = np.zeros((entries, 2), np.uint64)
    idx = (first + np.arange(n)) & (entries - 1)
    descs[idx, 0] = perm.astype(np.uint64) * np.uint64(C3D_CHUNK) + np.uint64(C3D_HEADROOM)
    descs[idx, 1] = lens.astype(np.uint64)
    d_descs, d_verd = f.alloc(descs.nbytes), f.alloc(n)
    d_descs.upload(descs)
    setup_s = time.time() - t0
    print(f"[{tag}] set up {setup_s:.1f}s", file=sys.stderr, flush=True)
    return types.SimpleNamespace(f=f, n=n, n4=n4, nports=nports, stride=stride, data=data, lens=lens,
                                 perm=perm, d_umem=d_umem, d_descs=d_descs, d_verd=d_verd, entries=entries,
                                 first=first, setup_s=setup_s)


def run_c3d(args):
    w = c3d_workload(args, "c3d")
    f, n, n4, nports, stride, data, lens = w.f, w.n, w.n4, w.nports, w.stride, w.data, w.lens
    d_umem, d_descs, d_verd, entries, first, setup_s = (w.d_umem, w.d_descs, w.d_verd, w.entries,
                                                        w.first, w.setup_s)

    def descs_ms():
        a = (d_umem.ptr, d_descs.ptr, n, d_verd.ptr)
        f.classify_descs_timed(*a, 2, first=first, mask=entries - 1)
        return f.classify_descs_timed(*a, args.iters, first=first, mask=entries - 1), f.last_path()

    def mpps(ms):
        return round(n / (ms * 1e-3) / 1e6, 1)

    runs = max(1, args.runs)
    new = [descs_ms() for _ in range(runs)]
    line = {"config": "c3d", "program": f.prog_name, "packets": n, "umem_chunk": C3D_CHUNK,
            "headroom": C3D_HEADROOM, "ring_entries": entries, "rules_ipv4": n4,
            "port_rules": nports, "kernel_path": new[0][1],
            "kernel_ms": [round(m, 4) for m, _ in new], "Mpps": [mpps(m) for m, _ in new],
            "setup_s": round(setup_s, 1)}
    if os.environ.get("XFG_LIB") == "diag":
        # the diagnostics library reads its knobs at every launch
        os.environ["XFG_KERNEL"] = "general"
        old = [descs_ms() for _ in range(runs)]
        del os.environ["XFG_KERNEL"]
        line["general"] = {"kernel_path": old[0][1], "kernel_ms": [round(m, 4) for m, _ in old],
                           "Mpps": [mpps(m) for m, _ in old]}
        line["speedup_vs_general"] = round(min(m for m, _ in old) / min(m for m, _ in new), 3)
        # the same frames as a strided batch: the generic pipelined kernel
        # (key mode 0) and the kernel C3 runs (the quotient index)
        d_data, d_lens = f.alloc(data.nbytes), f.alloc(lens.nbytes)
        d_data.upload(data)
        d_lens.upload(lens)
        for key, knob in (("strided_generic", "generic"), ("strided_qt", None)):
            if knob:
                os.environ["XFG_KERNEL"] = knob
            f.classify_timed(d_data.ptr, d_lens.ptr, n, stride, d_verd.ptr, 2)
            ms = [f.classify_timed(d_data.ptr, d_lens.ptr, n, stride, d_verd.ptr, args.iters)
                  for _ in range(runs)]
            line[key] = {"kernel_path": f.last_path(), "kernel_ms": [round(m, 4) for m in ms],
                         "Mpps": [mpps(m) for m in ms]}
            os.environ.pop("XFG_KERNEL", None)
    f.close()
    print(json.dumps(line), flush=True)


def run_c3f(args):
    """c3d's batch classified, then its egress (xfg_ring_egress): TX records
    of the PASS frames, fill addresses of the rest.  Each leg is args.iters
    launches between two events on a caller stream, args.runs times."""
    import numpy as np
    import torch
    import xfgpu as G
    w = c3d_workload(args, "c3f")
    f, n, entries, first = w.f, w.n, w.entries, w.first
    f.classify_descs(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, first=first, mask=entries - 1)
    f.sync()
    npass = int(np.count_nonzero(w.d_verd.download(np.zeros(n, np.uint8)) == 2))
    # TX and fill rings of the batch's size, each wrapping inside it
    d_tx, d_fill, d_idx, d_c = f.alloc(16 * n), f.alloc(8 * n), f.alloc(4 * n), f.alloc(16)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def egress(flags):
        f.ring_egress(w.d_descs.ptr, n, w.d_verd.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                      rx_first=first, rx_mask=entries - 1, tx_first=n - 777, tx_mask=n - 1,
                      fill_first=n - 555, fill_mask=n - 1, umem_ptr=w.d_umem.ptr, flags=flags,
                      stream=sp)

    legs = {"compact": lambda: f.compact(w.d_verd.ptr, n, 2, d_idx.ptr, d_c.ptr, stream=sp),
            "egress": lambda: egress(0),
            "egress_swap_macs": lambda: egress(G.EGRESS_SWAP_MACS)}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    runs = max(1, args.runs)
    ms = {k: [] for k in legs}
    for _ in range(runs):      # the legs interleaved
        for k, call in legs.items():
            ms[k].append(timed(call))
    counts = d_c.download(np.zeros(2, np.uint64)).tolist()
    assert counts == [npass, n - npass], counts
    # this device's own streaming-read rate, over the UMEM's first GiB
    probe = min(n * C3D_CHUNK, 1 << 30)
    f.stream_read_timed(w.d_umem.ptr, probe, 2)
    read_gbs = probe / (f.stream_read_timed(w.d_umem.ptr, probe, args.iters) * 1e-3) / 1e9
    # bytes the algorithm moves: a record and a verdict byte read a packet,
    # a TX record or a fill address written; the swap reads and writes 16 B
    # of every PASS frame
    moved = {"compact": n + 4 * npass, "egress": 17 * n + 16 * npass + 8 * (n - npass)}
    moved["egress_swap_macs"] = moved["egress"] + 32 * npass
    line = {"config": "c3f", "program": f.prog_name, "packets": n, "pass_frames": npass,
            "ring_entries": entries, "iters": args.iters, "stream_read_GBps": round(read_gbs, 1),
            "setup_s": round(w.setup_s, 1)}
    for k in legs:
        best = min(ms[k])
        gbs = moved[k] / (best * 1e-3) / 1e9
        line[k] = {"ms": [round(m, 4) for m in ms[k]], "bytes": moved[k], "GBps": round(gbs, 1),
                   "frac_of_stream_read": round(gbs / read_gbs, 3)}
    f.close()
    print(json.dumps(line), flush=True)


def run_c3st(args):
    """c3f's batch classified, then steered (xfg_steer_egress): the PASS frames
    over 1, 8 and 64 workers' TX rings by L4_HASH and by L4_DPORT, beside
    xfg_ring_egress on the same batch and verdicts.  Legs timed as c3f's."""
    import numpy as np
    import torch
    import xfgpu as G
    w = c3d_workload(args, "c3st")
    f, n, entries, first = w.f, w.n, w.entries, w.first
    f.classify_descs(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, first=first, mask=entries - 1)
    f.sync()
    npass = int(np.count_nonzero(w.d_verd.download(np.zeros(n, np.uint8)) == 2))
    kmax = 64
    d_tx, d_fill, d_c = f.alloc(16 * n * kmax), f.alloc(8 * n), f.alloc(8 * (kmax + 2))
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def egress():
        f.ring_egress(w.d_descs.ptr, n, w.d_verd.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                      rx_first=first, rx_mask=entries - 1, tx_first=n - 777, tx_mask=n - 1,
                      fill_first=n - 555, fill_mask=n - 1, stream=sp)

    def steer(k, mode):
        queues = G.steer_queues([(d_tx.ptr + 16 * n * q, n - 777 + q, n - 1) for q in range(k)])
        return lambda: f.steer_egress(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, d_c.ptr, queues,
                                      mode=mode, fill_ptr=d_fill.ptr, rx_first=first,
                                      rx_mask=entries - 1, fill_first=n - 555, fill_mask=n - 1,
                                      stream=sp)

    legs = {"ring_egress": egress}
    for k in (1, 8, 64):
        legs[f"steer_hash_k{k}"] = steer(k, G.STEER_L4_HASH)
        legs[f"steer_dport_k{k}"] = steer(k, G.STEER_L4_DPORT)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    runs = max(1, args.runs)
    ms = {k: [] for k in legs}
    spread = {}
    for r in range(runs):      # the legs interleaved
        for k, call in legs.items():
            ms[k].append(timed(call))
            if r == 0 and k != "ring_egress":
                nq = int(k.rsplit("k", 1)[1])
                c = d_c.download(np.zeros(nq + 2, np.uint64)).astype(np.int64)
                assert int(c[:nq].sum()) == npass and int(c[nq]) == n - npass, c
                spread[k] = {"min": int(c[:nq].min()), "max": int(c[:nq].max()), "refused": int(c[nq + 1])}
    # bytes the algorithm moves beyond xfg_ring_egress's: the header line (64
    # bytes) of every PASS frame
    base = 17 * n + 16 * npass + 8 * (n - npass)
    line = {"config": "c3st", "program": f.prog_name, "packets": n, "pass_frames": npass,
            "ring_entries": entries, "umem_chunk": C3D_CHUNK, "iters": args.iters,
            "setup_s": round(w.setup_s, 1)}
    ref = min(ms["ring_egress"])
    for k in legs:
        best = min(ms[k])
        moved = base + (0 if k == "ring_egress" else 64 * npass)
        line[k] = {"ms": [round(m, 4) for m in ms[k]], "bytes": moved,
                   "GBps": round(moved / (best * 1e-3) / 1e9, 1), "vs_ring_egress": round(best / ref, 2)}
        if k in spread:
            line[k]["queue_records"] = spread[k]
    f.close()
    print(json.dumps(line), flush=True)


def c3fw_fib(f, G, nroutes, nports):
    """A FIB of a default route and up to nroutes - 1 distinct random routes,
    80% of them /24 and 20% /25../32, over 4 next hops a port.  The longer ones
    lie in 2^14 /24s: the entry format holds 2^15 second-level groups."""
    import numpy as np
    rng = np.random.default_rng(20)
    nnh = 4 * nports
    length = np.where(rng.random(nroutes) < 0.8, 24, rng.integers(25, 33, nroutes))
    prefix = rng.integers(0, 1 << 32, nroutes)
    homes = rng.integers(0, 1 << 24, 1 << 14) << 8
    prefix = np.where(length > 24, homes[rng.integers(0, len(homes), nroutes)] | (prefix & 0xff), prefix)
    prefix &= (0xffffffff << (32 - length)) & 0xffffffff
    key = np.unique((prefix << 6) | length)[:max(nroutes - 1, 0)]
    routes = np.empty((len(key) + 1, 3), np.int64)
    routes[0] = (0, 0, 0)
    routes[1:, 0], routes[1:, 1] = key >> 6, key & 63
    routes[1:, 2] = rng.integers(0, nnh, len(key))
    nexthops = [(10 + k % nports, 0, 0, bytes([2, 1, 0, 0, 0, k]), bytes([2, 2, 0, 0, 0, k]))
                for k in range(nnh)]
    return G.Fib(f, routes, nexthops), len(routes)


def run_c3fw(args):
    """c3d's batch classified, then forwarded over 8 ports by a large FIB and
    by a default route alone, beside the steer call at K = 8 and the ring
    egress with the MAC swap.  Legs timed as c3f's."""
    import numpy as np
    import torch
    import xfgpu as G
    w = c3d_workload(args, "c3fw")
    f, n, entries, first = w.f, w.n, w.entries, w.first
    f.classify_descs(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, first=first, mask=entries - 1)
    f.sync()
    npass = int(np.count_nonzero(w.d_verd.download(np.zeros(n, np.uint8)) == 2))
    P = 8
    ncounts = P + 2 + G.FWD_REASONS
    d_tx, d_fill, d_c = f.alloc(16 * n * (P + 1)), f.alloc(8 * n), f.alloc(8 * ncounts)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    rings = [(d_tx.ptr + 16 * n * q, n - 777 + q, n - 1) for q in range(P + 1)]
    ports = G.fwd_ports([(10 + q,) + rings[q] for q in range(P)])
    queues = G.steer_queues(rings[:P])
    fibs = {"forward_2p20": c3fw_fib(f, G, 1 << 20, P), "forward_default": c3fw_fib(f, G, 1, P)}

    def forward(fib):
        return lambda: f.forward_egress(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, d_c.ptr, fib, ports,
                                        rings[P], fill_ptr=d_fill.ptr, rx_first=first,
                                        rx_mask=entries - 1, fill_first=n - 555, fill_mask=n - 1, stream=sp)

    legs = {k: forward(fib) for k, (fib, _) in fibs.items()}
    legs["steer_hash_k8"] = lambda: f.steer_egress(
        w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, d_c.ptr, queues, mode=G.STEER_L4_HASH,
        fill_ptr=d_fill.ptr, rx_first=first, rx_mask=entries - 1, fill_first=n - 555, fill_mask=n - 1,
        stream=sp)
    legs["ring_egress_swap"] = lambda: f.ring_egress(
        w.d_descs.ptr, n, w.d_verd.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr, rx_first=first,
        rx_mask=entries - 1, tx_first=n - 777, tx_mask=n - 1, fill_first=n - 555, fill_mask=n - 1,
        umem_ptr=w.d_umem.ptr, flags=G.EGRESS_SWAP_MACS, stream=sp)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def reasons():
        c = d_c.download(np.zeros(ncounts, np.uint64)).astype(np.int64)
        assert int(c[:P + 1].sum()) == npass and int(c[P + 1]) == n - npass, c
        return {"ports": c[:P].tolist(), "stack": int(c[P]), "reasons": c[P + 2:].tolist()}

    runs = max(1, args.runs)
    ms = {k: [] for k in legs}
    seen = {}
    for r in range(runs):      # the legs interleaved
        for k, call in legs.items():
            if r == 0 and k in fibs:
                call()
                torch.cuda.synchronize()
                seen[k] = {"first_call": reasons()}
            t = timed(call)
            if k in fibs:
                # every call decrements the forwarded frames' TTL: a run counts
                # only while the frames forwarded are the first call's
                last = reasons()
                seen[k].setdefault("forwarded_after_run", []).append(last["reasons"][0])
                if last != seen[k]["first_call"]:
                    continue
            ms[k].append(t)
    line = {"config": "c3fw", "program": f.prog_name, "packets": n, "pass_frames": npass, "ports": P,
            "ring_entries": entries, "umem_chunk": C3D_CHUNK, "iters": args.iters,
            "routes": {k: nr for k, (_, nr) in fibs.items()}, "setup_s": round(w.setup_s, 1)}
    ref = min(ms["steer_hash_k8"])
    for k in legs:
        best = min(ms[k])
        line[k] = {"ms": [round(m, 4) for m in ms[k]], "vs_steer_hash_k8": round(best / ref, 2)}
        line[k].update(seen.get(k, {}))
    line["table_cost_ms"] = round(min(ms["forward_2p20"]) - min(ms["forward_default"]), 4)
    for fib, _ in fibs.values():
        fib.free()
    f.close()
    print(json.dumps(line), flush=True)


def run_c3ch(args):
    """c3d's batch as a chained second stage, half the frames selected."""
    import numpy as np
    import torch
    w = c3d_workload(args, "c3ch")
    f, n, entries, first = w.f, w.n, w.entries, w.first
    ring = dict(first=first, mask=entries - 1)
    runs = max(1, args.runs)
    d_idx, d_c, d_half = f.alloc(4 * n), f.alloc(16), f.alloc(16 * (n // 2))
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    recs = np.zeros((n, 2), np.uint64)
    recs[:, 0] = w.perm.astype(np.uint64) * np.uint64(C3D_CHUNK) + np.uint64(C3D_HEADROOM)
    recs[:, 1] = w.lens.astype(np.uint64)

    def on_stream(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    f.classify_descs_timed(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, 2, **ring)
    whole = [f.classify_descs_timed(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, args.iters, **ring)
             for _ in range(runs)]
    line = {"config": "c3ch", "program": f.prog_name, "packets": n, "selected": n // 2,
            "ring_entries": entries, "iters": args.iters, "runs": runs,
            "classify_descs_whole_ms": [round(m, 4) for m in whole], "setup_s": round(w.setup_s, 1)}
    for name in ("alternating", "contiguous"):
        pre = np.ones(n, np.uint8)                 # DROP: not selected by XFG_CHAIN_PASS
        if name == "alternating":
            pre[0::2] = 2
        else:
            pre[n // 4:n // 4 + n // 2] = 2
        sel = np.flatnonzero(pre == 2)
        assert len(sel) == n // 2
        d_half.upload(recs[sel])
        f.classify_descs_timed(w.d_umem.ptr, d_half.ptr, n // 2, d_idx.ptr, 2)
        floor = [f.classify_descs_timed(w.d_umem.ptr, d_half.ptr, n // 2, d_idx.ptr, args.iters)
                 for _ in range(runs)]
        floor_path = f.last_path()
        w.d_verd.upload(pre)
        compact = [on_stream(lambda: f.compact(w.d_verd.ptr, n, 2, d_idx.ptr, d_c.ptr, stream=sp))
                   for _ in range(runs)]
        steps, ret_ms, end_ms = [], [], []
        for k in range(runs + 1):                  # (the first call grows the scratch: not counted)
            w.d_verd.upload(pre)
            f.sync()
            counts, ms = f.classify_descs_chain_timed(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, **ring)
            assert counts == (n // 2, n - n // 2), counts
            w.d_verd.upload(pre)
            f.sync()
            t0 = time.perf_counter()
            f.classify_descs_chain(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, **ring)
            t1 = time.perf_counter()
            f.sync()
            t2 = time.perf_counter()
            if k:
                steps.append([round(m, 4) for m in ms])
                ret_ms.append(round((t1 - t0) * 1e3, 4))
                end_ms.append(round((t2 - t0) * 1e3, 4))
        nsel = n // 2
        best = [min(s[j] for s in steps) for j in range(3)]
        sel_bytes, cmp_bytes = n + 16 * nsel + 16 * nsel + 4 * nsel, n + 4 * nsel
        line[name] = {
            "chain_steps_ms": steps, "chain_path": f.last_path(),
            "chain_wall_to_return_ms": ret_ms, "chain_wall_to_stream_end_ms": end_ms,
            "classify_descs_selected_half_ms": [round(m, 4) for m in floor], "floor_path": floor_path,
            "compact_ms": [round(m, 4) for m in compact],
            "overhead_over_floor_ms": round(min(end_ms) - min(floor), 4),
            "select_plus_scatter_ms": round(best[0] + best[2], 4),
            "select_bytes": sel_bytes, "compact_bytes": cmp_bytes,
            "select_GBps": round(sel_bytes / (best[0] * 1e-3) / 1e9, 1),
            "compact_GBps": round(cmp_bytes / (min(compact) * 1e-3) / 1e9, 1),
            "select_over_compact": round(best[0] / min(compact), 3)}
    f.close()
    print(json.dumps(line), flush=True)


def run_c3c(args):
    """c3d's batch classified, then its DROP frames captured whole as pcapng
    blocks (xfg_capture_descs), beside xfg_compact on the same verdicts; then
    the same ring with every frame 1514 bytes long, one frame in ten selected,
    cut to 96 bytes; and a one-tile batch for the fixed cost of a call.  Each
    leg is args.iters launches between two events on a caller stream."""
    import numpy as np
    import torch
    import xfgpu as G
    w = c3d_workload(args, "c3c")
    f, n, entries, first = w.f, w.n, w.entries, w.first
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    f.classify_descs(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr, first=first, mask=entries - 1)
    f.sync()
    verd = w.d_verd.download(np.zeros(n, np.uint8))
    ndrop = int(np.count_nonzero(verd == 1))
    # second setting: the same chunks, 1514-byte frames, 10 % DROP
    rng = np.random.default_rng(13)
    verd10 = np.where(rng.random(n) < 0.1, 1, 2).astype(np.uint8)
    n10 = int(np.count_nonzero(verd10 == 1))
    descs = w.d_descs.download(np.zeros((entries, 2), np.uint64))
    descs[:, 1] = 1514
    d_descs10, d_verd10 = f.alloc(descs.nbytes), f.alloc(n)
    d_descs10.upload(descs)
    d_verd10.upload(verd10)
    blk = 52 + ((w.lens.astype(np.int64) + 3) & ~3)
    total = int(blk[verd == 1].sum())
    total10 = n10 * (52 + 96)
    room = max(total, total10, 16)
    d_out, d_c, d_idx = f.alloc(room), f.alloc(32), f.alloc(4 * n)
    small = min(n, 2048)

    def capture(d_descs, d_verd, count, snaplen):
        b = G.DescBatch(w.d_umem.ptr, d_descs.ptr, first, entries - 1, count)
        return lambda: f.capture_into(b, d_verd.ptr, 1 << 1, d_out.ptr, room, d_c.ptr,
                                      snaplen=snaplen, stream=sp)

    legs = {"classify": lambda: f.classify_descs(w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr,
                                                 first=first, mask=entries - 1, stream=sp),
            "compact": lambda: f.compact(w.d_verd.ptr, n, 1, d_idx.ptr, d_c.ptr, stream=sp),
            "capture": capture(w.d_descs, w.d_verd, n, 0),
            "capture_1514_snap96_10pct": capture(d_descs10, d_verd10, n, 96),
            "capture_one_tile": capture(w.d_descs, w.d_verd, small, 0)}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    runs = max(1, args.runs)
    ms = {k: [] for k in legs}
    got = {}
    for _ in range(runs):      # the legs interleaved
        for k, call in legs.items():
            ms[k].append(timed(call))
            got[k] = d_c.download(np.zeros(3, np.uint64)).tolist()
    assert got["capture"] == [ndrop, total, 0], got["capture"]
    assert got["capture_1514_snap96_10pct"] == [n10, total10, 0], got
    probe = min(n * C3D_CHUNK, 1 << 30)
    f.stream_read_timed(w.d_umem.ptr, probe, 2)
    read_gbs = probe / (f.stream_read_timed(w.d_umem.ptr, probe, args.iters) * 1e-3) / 1e9
    # bytes the algorithm moves: a verdict byte a packet; a 16-byte record and
    # the captured payload (to the dword) of a selected frame read, its block
    # written
    moved = {"compact": n + 4 * ndrop,
             "capture": n + 16 * ndrop + (total - 52 * ndrop) + total,
             "capture_1514_snap96_10pct": n + 16 * n10 + 96 * n10 + total10}
    line = {"config": "c3c", "program": f.prog_name, "packets": n, "drop_frames": ndrop,
            "capture_bytes": total, "selected_10pct": n10, "capture_bytes_10pct": total10,
            "one_tile_packets": small, "iters": args.iters,
            "stream_read_GBps": round(read_gbs, 1), "setup_s": round(w.setup_s, 1)}
    for k in legs:
        line[k] = {"ms": [round(m, 4) for m in ms[k]]}
        if k in moved:
            gbs = moved[k] / (min(ms[k]) * 1e-3) / 1e9
            line[k].update(bytes=moved[k], GBps=round(gbs, 1),
                           frac_of_stream_read=round(gbs / read_gbs, 3))
    line["capture_share_of_classify"] = round(min(ms["capture"]) / min(ms["classify"]), 3)
    f.close()
    print(json.dumps(line), flush=True)


def c3m_workload(args, name):
    """c3m's batch on the device, classified once by xfg_classify_descs_frags
    and checked against c3d's verdicts of the heads (shared by c3m and c3mc)."""
    import types
    import numpy as np
    import xfgpu as G
    w = c3d_workload(args, name, umem_chunks=3)
    f, n, stride = w.f, w.n, w.stride
    t0 = time.time()
    # c3d on the heads alone, and their verdicts: the frames that hit a rule
    a = (w.d_umem.ptr, w.d_descs.ptr, n, w.d_verd.ptr)
    f.classify_descs_timed(*a, 2, first=w.first, mask=w.entries - 1)
    runs = max(1, args.runs)
    c3d_ms = [f.classify_descs_timed(*a, args.iters, first=w.first, mask=w.entries - 1)
              for _ in range(runs)]
    c3d_path = f.last_path()
    hv = w.d_verd.download(np.zeros(n, np.uint8))
    hit = np.flatnonzero(hv == 2)[:4096]          # (deny program: a hit passes)
    assert len(hit) >= 16, "no frames that hit a rule"
    frames = w.data.reshape(n, stride)
    # continuation chunk c (of 2n, past the heads' chunks) holds a hit frame
    rng = np.random.default_rng(14)
    cperm = rng.permutation(2 * n)                # continuation k of packet i: chunk n + cperm[2i + k]
    which = hit[rng.integers(0, len(hit), 2 * n)]
    cinv = np.empty(2 * n, np.int64)
    cinv[cperm] = np.arange(2 * n)
    piece = 1 << 17
    buf = np.zeros((piece, C3D_CHUNK), np.uint8)
    for c0 in range(0, 2 * n, piece):
        c1 = min(2 * n, c0 + piece)
        buf[:c1 - c0, C3D_HEADROOM:C3D_HEADROOM + stride] = frames[which[cinv[c0:c1]]]
        G._check(G.lib.xfg_memcpy_h2d(f.ctx, 0, w.d_umem.ptr + (n + c0) * C3D_CHUNK, buf.ctypes.data,
                                      (c1 - c0) * C3D_CHUNK), "memcpy_h2d")
    nrec = 3 * n
    entries = 1 << (nrec - 1).bit_length()
    first = entries - 777
    rec = np.zeros((n, 3, 2), np.uint64)
    rec[:, 0, 0] = w.perm.astype(np.uint64) * np.uint64(C3D_CHUNK) + np.uint64(C3D_HEADROOM)
    rec[:, 0, 1] = w.lens.astype(np.uint64) | np.uint64(G.XDP_PKT_CONTD << 32)
    for k in (1, 2):
        rec[:, k, 0] = (n + cperm[k - 1::2]).astype(np.uint64) * np.uint64(C3D_CHUNK) + np.uint64(C3D_HEADROOM)
        rec[:, k, 1] = w.lens[which[cinv[cperm[k - 1::2]]]].astype(np.uint64) | \
            np.uint64((G.XDP_PKT_CONTD if k == 1 else 0) << 32)
    descs = np.zeros((entries, 2), np.uint64)
    descs[(first + np.arange(nrec)) & (entries - 1)] = rec.reshape(nrec, 2)
    d_descs, d_verd, d_pkt = f.alloc(descs.nbytes), f.alloc(nrec), f.alloc(4 * nrec)
    d_descs.upload(descs)
    del descs, rec, buf
    print(f"[{name}] continuations set up {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    fa = (w.d_umem.ptr, d_descs.ptr, nrec, d_verd.ptr)
    fk = dict(pkt_of_ptr=d_pkt.ptr, first=first, mask=entries - 1)
    f.stats_reset()
    counts = f.classify_descs_frags(*fa, **fk)
    f.sync()
    assert counts == (n, nrec, 0), counts
    # the heads' verdicts on every record of their packets, and only the heads counted
    v = d_verd.download(np.zeros(nrec, np.uint8)).reshape(n, 3)
    assert np.array_equal(v, np.repeat(hv[:, None], 3, axis=1)), "verdicts differ from c3d's"
    st = f.stats()
    assert int(st[:, 0].sum()) == n, st
    frags_path = f.last_path()
    return types.SimpleNamespace(w=w, t0=t0, runs=runs, c3d_ms=c3d_ms, c3d_path=c3d_path, hv=hv,
                                 nrec=nrec, entries=entries, first=first, d_descs=d_descs,
                                 d_verd=d_verd, d_pkt=d_pkt, fa=fa, fk=fk, v=v,
                                 frags_path=frags_path)


def run_c3mst(args):
    """c3m's batch classified by xfg_classify_descs_frags, then steered by whole
    packets (xfg_steer_frags_egress) over 1, 8 and 64 workers' TX rings by
    L4_HASH and by L4_DPORT, beside xfg_ring_egress with XFG_EGRESS_MULTIBUF on
    the same records and verdicts; and the same records with XDP_PKT_CONTD
    cleared (every record its own packet) through xfg_steer_egress and
    xfg_steer_frags_egress over 8 rings.  Legs timed as c3st's."""
    import numpy as np
    import torch
    import xfgpu as G
    cm = c3m_workload(args, "c3mst")
    w, nrec, entries, first = cm.w, cm.nrec, cm.entries, cm.first
    f, n = w.f, w.n
    npass = int(np.count_nonzero(cm.hv == 2))     # PASS packets: three TX records each
    kmax = 64
    d_tx, d_fill, d_c = f.alloc(16 * entries * kmax), f.alloc(8 * entries), f.alloc(8 * (kmax + 2))
    # the all-end-of-packet batch: the same records, the option words cleared
    descs = cm.d_descs.download(np.zeros((entries, 2), np.uint64))
    descs[:, 1] &= np.uint64(0xffffffff)
    d_eop = f.alloc(descs.nbytes)
    d_eop.upload(descs)
    del descs
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    ring = dict(rx_first=first, rx_mask=entries - 1, fill_first=entries - 555, fill_mask=entries - 1)

    def egress():
        f.ring_egress(cm.d_descs.ptr, nrec, cm.d_verd.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                      tx_first=entries - 777, tx_mask=entries - 1, flags=G.EGRESS_MULTIBUF, stream=sp, **ring)

    def steer(call, d_rx, k, mode):
        queues = G.steer_queues([(d_tx.ptr + 16 * entries * q, entries - 777 + q, entries - 1)
                                 for q in range(k)])
        return lambda: call(w.d_umem.ptr, d_rx.ptr, nrec, cm.d_verd.ptr, d_c.ptr, queues, mode=mode,
                            fill_ptr=d_fill.ptr, stream=sp, **ring)

    legs = {"ring_egress_multibuf": egress}
    for k in (1, 8, 64):
        legs[f"steer_frags_hash_k{k}"] = steer(f.steer_frags_egress, cm.d_descs, k, G.STEER_L4_HASH)
        legs[f"steer_frags_dport_k{k}"] = steer(f.steer_frags_egress, cm.d_descs, k, G.STEER_L4_DPORT)
    legs["all_eop_steer_hash_k8"] = steer(f.steer_egress, d_eop, 8, G.STEER_L4_HASH)
    legs["all_eop_steer_frags_hash_k8"] = steer(f.steer_frags_egress, d_eop, 8, G.STEER_L4_HASH)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    runs = max(1, args.runs)
    ms = {k: [] for k in legs}
    spread = {}
    for r in range(runs):      # the legs interleaved
        for k, call in legs.items():
            ms[k].append(timed(call))
            if r == 0 and k != "ring_egress_multibuf":
                nq = int(k.rsplit("k", 1)[1])
                c = d_c.download(np.zeros(nq + 2, np.uint64)).astype(np.int64)
                if k.startswith("steer_frags"):
                    assert int(c[:nq].sum()) == 3 * npass and int(c[nq]) == nrec - 3 * npass, c
                else:
                    assert int(c[:nq + 1].sum()) == nrec, c
                spread[k] = {"min": int(c[:nq].min()), "max": int(c[:nq].max()), "refused": int(c[nq + 1])}
    # the two calls agree on the all-end-of-packet batch
    assert spread["all_eop_steer_hash_k8"] == spread["all_eop_steer_frags_hash_k8"], spread
    # bytes the algorithm moves: a verdict byte and a 16-byte record a record
    # in, a TX record (16) or a fill address (8) out; steering reads the header
    # line (64 bytes) of every PASS head, a third of the PASS records here
    base = 17 * nrec + 16 * 3 * npass + 8 * (nrec - 3 * npass)
    line = {"config": "c3mst", "program": f.prog_name, "packets": n, "records": nrec,
            "pass_packets": npass, "ring_entries": entries, "umem_chunk": C3D_CHUNK, "iters": args.iters,
            "setup_s": round(w.setup_s + time.time() - cm.t0, 1)}
    ref = min(ms["ring_egress_multibuf"])
    for k in legs:
        best = min(ms[k])
        line[k] = {"ms": [round(m, 4) for m in ms[k]], "vs_ring_egress_multibuf": round(best / ref, 2)}
        if not k.startswith("all_eop"):
            moved = base + (0 if k == "ring_egress_multibuf" else 64 * npass)
            line[k].update(bytes=moved, GBps=round(moved / (best * 1e-3) / 1e9, 1))
        if k in spread:
            line[k]["queue_records"] = spread[k]
    line["all_eop_frags_vs_single"] = round(min(ms["all_eop_steer_frags_hash_k8"]) /
                                            min(ms["all_eop_steer_hash_k8"]), 3)
    f.close()
    print(json.dumps(line), flush=True)


def run_c3mfw(args):
    """c3m's batch classified by xfg_classify_descs_frags, then forwarded by
    whole packets (xfg_forward_frags_egress) over 8 ports by a 2^20-route FIB
    and by a default route alone, beside xfg_ring_egress with
    XFG_EGRESS_MULTIBUF on the same records and verdicts; and the same records
    with XDP_PKT_CONTD cleared (every record its own packet) through
    xfg_forward_egress and xfg_forward_frags_egress: the price of the new
    kernel where the old one could be used.  Legs timed as c3fw's, with its
    rule for the runs after which fewer frames are forwarded."""
    import numpy as np
    import torch
    import xfgpu as G
    cm = c3m_workload(args, "c3mfw")
    w, nrec, entries, first = cm.w, cm.nrec, cm.entries, cm.first
    f, n = w.f, w.n
    npass = int(np.count_nonzero(cm.hv == 2))     # PASS packets: three TX records each
    P = 8
    ncounts = P + 2 + G.FWD_REASONS
    d_tx, d_fill, d_c = f.alloc(16 * entries * (P + 1)), f.alloc(8 * entries), f.alloc(8 * ncounts)
    # the all-end-of-packet batch: the same records, the option words cleared
    descs = cm.d_descs.download(np.zeros((entries, 2), np.uint64))
    descs[:, 1] &= np.uint64(0xffffffff)
    d_eop = f.alloc(descs.nbytes)
    d_eop.upload(descs)
    del descs
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    ring = dict(rx_first=first, rx_mask=entries - 1, fill_first=entries - 555, fill_mask=entries - 1)
    rings = [(d_tx.ptr + 16 * entries * q, entries - 777 + q, entries - 1) for q in range(P + 1)]
    ports = G.fwd_ports([(10 + q,) + rings[q] for q in range(P)])
    fibs = {"2p20": c3fw_fib(f, G, 1 << 20, P), "default": c3fw_fib(f, G, 1, P)}

    def forward(call, d_rx, fib):
        return lambda: call(w.d_umem.ptr, d_rx.ptr, nrec, cm.d_verd.ptr, d_c.ptr, fib, ports, rings[P],
                            fill_ptr=d_fill.ptr, stream=sp, **ring)

    legs = {"ring_egress_multibuf": lambda: f.ring_egress(
        cm.d_descs.ptr, nrec, cm.d_verd.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
        tx_first=entries - 777, tx_mask=entries - 1, flags=G.EGRESS_MULTIBUF, stream=sp, **ring)}
    for k, (fib, _) in fibs.items():
        legs[f"forward_frags_{k}"] = forward(f.forward_frags_egress, cm.d_descs, fib)
    legs["all_eop_forward_2p20"] = forward(f.forward_egress, d_eop, fibs["2p20"][0])
    legs["all_eop_forward_frags_2p20"] = forward(f.forward_frags_egress, d_eop, fibs["2p20"][0])

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    def reasons(k):
        c = d_c.download(np.zeros(ncounts, np.uint64)).astype(np.int64)
        if k.startswith("all_eop"):
            assert int(c[:P + 2].sum()) == nrec and int(c[P + 2:].sum()) == 3 * npass, c
        else:
            # the rings count records, the reasons packets
            assert int(c[:P + 1].sum()) == 3 * npass and int(c[P + 1]) == nrec - 3 * npass, c
            assert int(c[P + 2:].sum()) == npass, c
        return {"ports": c[:P].tolist(), "stack": int(c[P]), "reasons": c[P + 2:].tolist()}

    runs = max(1, args.runs)
    ms = {k: [] for k in legs}
    every = {k: [] for k in legs}
    seen = {}
    for r in range(runs):      # the legs interleaved
        for k, call in legs.items():
            fwd = k != "ring_egress_multibuf"
            if r == 0 and fwd:
                call()
                torch.cuda.synchronize()
                seen[k] = {"first_call": reasons(k)}
            t = timed(call)
            every[k].append(t)
            if fwd:
                # every call decrements the forwarded heads' TTL: a run counts
                # only while the packets forwarded are the first call's
                last = reasons(k)
                seen[k].setdefault("forwarded_after_run", []).append(last["reasons"][0])
                if last != seen[k]["first_call"]:
                    continue
            ms[k].append(t)
    line = {"config": "c3mfw", "program": f.prog_name, "packets": n, "records": nrec,
            "pass_packets": npass, "ports": P, "ring_entries": entries, "umem_chunk": C3D_CHUNK,
            "iters": args.iters, "routes": {k: nr for k, (_, nr) in fibs.items()},
            "setup_s": round(w.setup_s + time.time() - cm.t0, 1)}
    for k in legs:
        if not ms[k]:          # no run left the first call's packets forwarded: all runs, marked
            ms[k] = every[k]
            seen[k]["no_run_kept_the_first_calls_packets"] = True
    ref = min(ms["ring_egress_multibuf"])
    for k in legs:
        best = min(ms[k])
        line[k] = {"ms": [round(m, 4) for m in ms[k]], "vs_ring_egress_multibuf": round(best / ref, 2)}
        line[k].update(seen.get(k, {}))
    line["table_cost_ms"] = round(min(ms["forward_frags_2p20"]) - min(ms["forward_frags_default"]), 4)
    line["all_eop_frags_vs_single"] = round(min(ms["all_eop_forward_frags_2p20"]) /
                                            min(ms["all_eop_forward_2p20"]), 3)
    for fib, _ in fibs.values():
        fib.free()
    f.close()
    print(json.dumps(line), flush=True)


def run_c3mc(args):
    """c3m's batch classified by xfg_classify_descs_frags, then its DROP
    packets captured whole (xfg_capture_descs_frags, snaplen 0), head only,
    and, over the same records and verdicts, record by record
    (xfg_capture_descs: the same payload bytes in three times the blocks).
    Each leg is args.iters launches between two events on a caller stream."""
    import numpy as np
    import torch
    import xfgpu as G
    cm = c3m_workload(args, "c3mc")
    w, nrec, entries, first, v = cm.w, cm.nrec, cm.entries, cm.first, cm.v
    f, n = w.f, w.n
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    descs = cm.d_descs.download(np.zeros((entries, 2), np.uint64))
    lens = (descs[(first + np.arange(nrec)) & (entries - 1), 1] & np.uint64(0xffffffff)) \
        .astype(np.int64).reshape(n, 3)
    del descs
    drop = v[:, 0] == 1
    ndrop = int(np.count_nonzero(drop))
    payload = int(lens[drop].sum())
    total = int((52 + ((lens[drop].sum(axis=1) + 3) & ~3)).sum())
    total_head = int((52 + ((lens[drop, 0] + 3) & ~3)).sum())
    total_recs = int((52 + ((lens[drop] + 3) & ~3)).sum())
    room = max(total, total_recs, 16)
    d_out, d_c = f.alloc(room), f.alloc(32)
    b = G.DescBatch(w.d_umem.ptr, cm.d_descs.ptr, first, entries - 1, nrec)
    legs = {"capture_frags": lambda: f.capture_frags_into(b, cm.d_verd.ptr, 1 << 1, d_out.ptr, room,
                                                          d_c.ptr, stream=sp),
            "capture_frags_head_only": lambda: f.capture_frags_into(
                b, cm.d_verd.ptr, 1 << 1, d_out.ptr, room, d_c.ptr, flags=G.CAPTURE_HEAD_ONLY,
                stream=sp),
            "capture_descs_same_records": lambda: f.capture_into(b, cm.d_verd.ptr, 1 << 1, d_out.ptr,
                                                                 room, d_c.ptr, stream=sp)}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    runs = max(1, args.runs)
    ms = {k: [] for k in legs}
    got = {}
    for _ in range(runs):      # the legs interleaved
        for k, call in legs.items():
            ms[k].append(timed(call))
            got[k] = d_c.download(np.zeros(3, np.uint64)).tolist()
    assert got["capture_frags"] == [ndrop, total, 0], got
    assert got["capture_frags_head_only"] == [ndrop, total_head, 0], got
    assert got["capture_descs_same_records"] == [3 * ndrop, total_recs, 0], got
    probe = min(n * C3D_CHUNK, 1 << 30)
    f.stream_read_timed(w.d_umem.ptr, probe, 2)
    read_gbs = probe / (f.stream_read_timed(w.d_umem.ptr, probe, args.iters) * 1e-3) / 1e9
    # bytes the algorithm moves.  Whole packets: the scan reads a verdict byte
    # and a 16-byte record a record, writes off[] (4) and, a packet, its head's
    # slot of tot[] (8) over the launch's fill (8 a record); the copy reads
    # tot[] (8 a record), a selected head's verdict byte, and for its block the
    # records (16 each), their off[] (4 each) and the payload, and writes the
    # block.  Record by record: as c3c states it.
    moved = {"capture_frags": nrec * (1 + 16 + 4 + 8 + 8) + 8 * n + ndrop * (1 + 3 * 20) +
             payload + total,
             "capture_descs_same_records": nrec + 16 * 3 * ndrop + payload + total_recs}
    line = {"config": "c3mc", "program": f.prog_name, "packets": n, "records": nrec,
            "drop_packets": ndrop, "payload_bytes": payload, "capture_bytes": total,
            "capture_bytes_head_only": total_head, "capture_bytes_record_by_record": total_recs,
            "iters": args.iters, "stream_read_GBps": round(read_gbs, 1),
            "setup_s": round(w.setup_s + time.time() - cm.t0, 1)}
    for k in legs:
        line[k] = {"ms": [round(m, 4) for m in ms[k]]}
        if k in moved:
            gbs = moved[k] / (min(ms[k]) * 1e-3) / 1e9
            line[k].update(bytes=moved[k], GBps=round(gbs, 1),
                           frac_of_stream_read=round(gbs / read_gbs, 3))
    line["frags_over_record_by_record"] = round(
        min(ms["capture_frags"]) / min(ms["capture_descs_same_records"]), 3)
    f.close()
    print(json.dumps(line), flush=True)


def run_c3mch(args):
    """c3m's batch as the second stage of a chain over multi-buffer packets,
    half the packets selected."""
    import numpy as np
    cm = c3m_workload(args, "c3mch")
    w, nrec, entries, first, runs = cm.w, cm.nrec, cm.entries, cm.first, cm.runs
    f, n = w.f, w.n
    ring = dict(first=first, mask=entries - 1)
    descs = cm.d_descs.download(np.zeros((entries, 2), np.uint64))
    recs = descs[(first + np.arange(nrec)) & (entries - 1)].reshape(n, 3, 2)
    del descs
    nsel = n // 2
    d_half, d_hv = f.alloc(16 * 3 * nsel), f.alloc(3 * nsel)
    line = {"config": "c3mch", "program": f.prog_name, "packets": n, "records": nrec,
            "selected_packets": nsel, "ring_entries": entries, "iters": args.iters, "runs": runs,
            "setup_s": round(w.setup_s + time.time() - cm.t0, 1)}
    for name in ("alternating", "contiguous"):
        pre = np.ones((n, 3), np.uint8)            # DROP: not selected by XFG_CHAIN_PASS
        if name == "alternating":
            pre[0::2] = 2
        else:
            pre[n // 4:n // 4 + nsel] = 2
        sel = np.flatnonzero(pre[:, 0] == 2)
        assert len(sel) == nsel
        # the floor: the selected packets alone, as a ring of their own
        d_half.upload(np.ascontiguousarray(recs[sel]))
        fl = (w.d_umem.ptr, d_half.ptr, 3 * nsel, d_hv.ptr)
        floor = []
        for k in range(runs + 1):
            counts, ms = f.classify_descs_frags_timed(*fl)
            assert counts == (nsel, 3 * nsel, 0), counts
            if k:
                floor.append([round(m, 4) for m in ms])
        floor_path = f.last_path()
        steps, ret_ms, end_ms = [], [], []
        for k in range(runs + 1):                  # (the first call grows the scratch: not counted)
            cm.d_verd.upload(pre)
            f.sync()
            counts, ms = f.classify_descs_frags_chain_timed(w.d_umem.ptr, cm.d_descs.ptr, nrec,
                                                            cm.d_verd.ptr, **ring)
            assert counts == (nsel, 3 * nsel, nrec - 3 * nsel), counts
            got = cm.d_verd.download(np.zeros(nrec, np.uint8)).reshape(n, 3)
            want = pre.copy()
            want[sel] = cm.hv[sel, None]
            assert np.array_equal(got, want), "verdicts differ from c3d's of the selected heads"
            cm.d_verd.upload(pre)
            f.sync()
            t0 = time.perf_counter()
            f.classify_descs_frags_chain(w.d_umem.ptr, cm.d_descs.ptr, nrec, cm.d_verd.ptr, **ring)
            t1 = time.perf_counter()
            f.sync()
            t2 = time.perf_counter()
            if k:
                steps.append([round(m, 4) for m in ms])
                ret_ms.append(round((t1 - t0) * 1e3, 4))
                end_ms.append(round((t2 - t0) * 1e3, 4))
        best = [min(s[j] for s in steps) for j in range(3)]
        fbest = [min(s[j] for s in floor) for j in range(3)]
        # bytes the two pre-pass kernels move: a verdict byte and the options a
        # record, seg_of out, the fill and the read-back of head_of_seg and
        # end_of_seg, rank_of_seg out; a head's index and its end a packet; a
        # verdict byte, the head record in and out and idx a selected packet
        pre_bytes = nrec * (1 + 4 + 4 + 8 + 8 + 4) + 8 * n + nsel * (1 + 16 + 16 + 4)
        spread_bytes = nrec * (4 + 4) + 3 * nsel * 2 + nsel
        line[name] = {
            "frags_chain_steps_ms": steps, "frags_chain_path": f.last_path(),
            "frags_chain_wall_to_return_ms": ret_ms, "frags_chain_wall_to_stream_end_ms": end_ms,
            "classify_descs_frags_selected_alone_steps_ms": floor, "floor_path": floor_path,
            "overhead_over_floor_ms": round(sum(best) - sum(fbest), 4),
            "prepass_plus_spread_ms": round(best[0] + best[2], 4),
            "prepass_bytes": pre_bytes, "spread_bytes": spread_bytes,
            "prepass_GBps": round(pre_bytes / (best[0] * 1e-3) / 1e9, 1),
            "spread_GBps": round(spread_bytes / (best[2] * 1e-3) / 1e9, 1)}
    f.close()
    print(json.dumps(line), flush=True)


def run_c3m(args):
    """c3d's frames as the heads of 3-record packets (see the module text)."""
    import numpy as np
    import torch
    import xfgpu as G
    cm = c3m_workload(args, "c3m")
    w, t0, runs, c3d_ms, c3d_path, nrec = cm.w, cm.t0, cm.runs, cm.c3d_ms, cm.c3d_path, cm.nrec
    entries, first, d_descs, d_verd, fa, fk = cm.entries, cm.first, cm.d_descs, cm.d_verd, cm.fa, cm.fk
    v, frags_path, f, n = cm.v, cm.frags_path, w.f, w.n
    steps = {"head_pass": [], "classify_heads": [], "spread": []}
    wall_return, wall_done = [], []
    for _ in range(runs):
        for _ in range(max(1, args.iters // 2)):
            _, ms = f.classify_descs_frags_timed(*fa, **fk)
            for k, m in zip(steps, ms):
                steps[k].append(m)
        f.sync()
        t1 = time.perf_counter()
        for _ in range(args.iters):
            f.classify_descs_frags(*fa, **fk)
        t2 = time.perf_counter()
        f.sync()
        t3 = time.perf_counter()
        wall_return.append((t2 - t1) / args.iters * 1e3)
        wall_done.append((t3 - t1) / args.iters * 1e3)
    # the egress of the 3n records, as c3f times its legs
    npass = int(np.count_nonzero(v == 2))
    te = 1 << (nrec - 1).bit_length()
    d_tx, d_fill, d_c = f.alloc(16 * te), f.alloc(8 * te), f.alloc(16)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def egress(flags):
        f.ring_egress(d_descs.ptr, nrec, d_verd.ptr, d_c.ptr, tx_ptr=d_tx.ptr, fill_ptr=d_fill.ptr,
                      rx_first=first, rx_mask=entries - 1, tx_first=te - 777, tx_mask=te - 1,
                      fill_first=te - 555, fill_mask=te - 1, umem_ptr=w.d_umem.ptr, flags=flags,
                      stream=sp)

    legs = {"egress": lambda: egress(0),
            "egress_multibuf": lambda: egress(G.EGRESS_MULTIBUF),
            "egress_multibuf_swap_macs": lambda: egress(G.EGRESS_MULTIBUF | G.EGRESS_SWAP_MACS)}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(2):
            call()
        e0.record(stream)
        for _ in range(args.iters):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    ems = {k: [] for k in legs}
    for _ in range(runs):
        for k, call in legs.items():
            ems[k].append(timed(call))
    ec = d_c.download(np.zeros(2, np.uint64)).tolist()
    assert ec == [npass, nrec - npass], ec
    best = {k: min(x) for k, x in steps.items()}
    line = {"config": "c3m", "program": f.prog_name, "packets": n, "records": nrec,
            "ring_entries": entries, "iters": args.iters,
            "kernel_path_heads": frags_path,
            "frags_ms": {k: round(m, 4) for k, m in best.items()},
            "frags_steps_sum_ms": round(sum(best.values()), 4),
            "frags_call_wall_ms": {"to_return": [round(m, 4) for m in wall_return],
                                   "to_stream_end": [round(m, 4) for m in wall_done]},
            "passes_over_classify": round((best["head_pass"] + best["spread"]) / best["classify_heads"], 3),
            "c3d_same_heads": {"kernel_path": c3d_path, "kernel_ms": [round(m, 4) for m in c3d_ms],
                               "Mpps": [round(n / (m * 1e-3) / 1e6, 1) for m in c3d_ms]},
            "Mpps_whole_call": round(n / (min(wall_done) * 1e-3) / 1e6, 1),
            "bytes": {"head_pass": 16 * nrec + 4 * nrec + 16 * n, "spread": 4 * nrec + nrec + n},
            "pass_records": npass, "setup_s": round(w.setup_s + time.time() - t0, 1)}
    for k in ("head_pass", "spread"):
        line["GBps_" + k] = round(line["bytes"][k] / (best[k] * 1e-3) / 1e9, 1)
    for k in legs:
        line[k] = {"ms": [round(m, 4) for m in ems[k]]}
    f.close()
    print(json.dumps(line), flush=True)


def run_c3s(args):
    """C3's rules and frames in a UMEM, scattered over S sockets of B records
    (a poll round of an application with a socket a NIC queue): the round as
    the per-ring calls make it -- xfg_classify_descs and xfg_ring_egress a
    socket, 2 S calls -- beside one xfg_classify_socks and one
    xfg_socks_egress.  Whole rounds by host wall clock, one xfg_sync at the end
    of a leg's run; the legs alternate, args.runs runs each.  The context keeps
    the default descs_min_packets, so either leg's classify takes the kernel a
    caller would get."""
    import ctypes as C
    import statistics
    import numpy as np
    import xfgpu as G
    points = ([(s, b) for b in (64, 256) for s in (4, 64, 1024)] if args.sweep
              else [(args.socks, args.batch)])
    most = max(s * b for s, b in points)
    w = c3d_workload(args, "c3s", log2_default=max(12, (most - 1).bit_length()), descs_min_packets=0)
    f = w.f
    assert most <= w.n, "more records than --log2-packets frames"
    for S, B in points:
        n, R = S * B, 2 * B                    # every ring twice the batch, wrapping inside it
        first = R - 7
        # socket s's RX ring: frames s * B .. of the workload, C3D's chunk addresses
        descs = np.zeros((S, R, 2), np.uint64)
        idx = (first + np.arange(B)) & (R - 1)
        addr = w.perm[:n].astype(np.uint64) * np.uint64(C3D_CHUNK) + np.uint64(C3D_HEADROOM)
        descs[:, idx, 0] = addr.reshape(S, B)
        descs[:, idx, 1] = w.lens[:n].astype(np.uint64).reshape(S, B)
        d_rx, d_tx, d_fill = f.alloc(descs.nbytes), f.alloc(16 * S * R), f.alloc(8 * S * R)
        d_v = [f.alloc(n), f.alloc(n)]
        d_c = [f.alloc(16 * S), f.alloc(8 * (2 * S + 2))]
        d_rx.upload(descs)
        rings = [dict(rx_descs=d_rx.ptr + 16 * R * s, rx_first=first, rx_mask=R - 1,
                      tx_descs=d_tx.ptr + 16 * R * s, tx_first=R - 5, tx_mask=R - 1,
                      fill_addrs=d_fill.ptr + 8 * R * s, fill_first=R - 3, fill_mask=R - 1, count=B)
                 for s in range(S)]
        # leg 1: the structures of every call built once, the library called directly
        per = []
        for s, r in enumerate(rings):
            db = G.DescBatch(w.d_umem.ptr, r["rx_descs"], first, R - 1, B)
            e = G.Egress(C.sizeof(G.Egress), None, r["rx_descs"], first, R - 1, r["tx_descs"],
                         r["tx_first"], R - 1, r["fill_addrs"], r["fill_first"], R - 1, B,
                         d_c[0].ptr + 16 * s, 0)
            per.append((C.byref(db), C.byref(e), d_v[0].ptr + s * B, db, e))
        tab = G.sock_table(rings)
        sk = G.Socks(C.sizeof(G.Socks), w.d_umem.ptr, tab, None, S)
        se = G.SocksEgress(C.sizeof(G.SocksEgress), None, 0, 0, d_c[1].ptr, 0)
        lib, ctx = G.lib, f.ctx

        def loop_round():
            for db, e, v, _, _ in per:
                rc = lib.xfg_classify_descs(ctx, 0, db, v, None) or lib.xfg_ring_egress(ctx, 0, e, v, None)
                assert rc == 0, rc

        def single_round():
            rc = (lib.xfg_classify_socks(ctx, 0, C.byref(sk), d_v[1].ptr, None) or
                  lib.xfg_socks_egress(ctx, 0, C.byref(sk), C.byref(se), d_v[1].ptr, None))
            assert rc == 0, rc

        legs = {"per_socket_loop": loop_round, "single_call": single_round}
        rounds, us, paths = {}, {k: [] for k in legs}, {}
        for k, one in legs.items():                 # warm-up, and how many rounds a run needs
            for _ in range(3):
                one()
            f.sync()
            t0 = time.perf_counter()
            for _ in range(3):
                one()
            f.sync()
            rounds[k] = int(min(2000, max(5, 0.1 / ((time.perf_counter() - t0) / 3))))
            paths[k] = f.last_path()
        for _ in range(max(1, args.runs)):
            for k, one in legs.items():
                t0 = time.perf_counter()
                for _ in range(rounds[k]):
                    one()
                f.sync()
                us[k].append((time.perf_counter() - t0) / rounds[k] * 1e6)
        # both legs computed the same round
        v0, v1 = (d.download(np.zeros(n, np.uint8)) for d in d_v)
        assert np.array_equal(v0, v1)
        c0 = d_c[0].download(np.zeros(2 * S, np.uint64))
        c1 = d_c[1].download(np.zeros(2 * S + 2, np.uint64))
        assert np.array_equal(c0, c1[:2 * S]) and int(c1[2 * S]) == int(np.count_nonzero(v1 == 2))
        line = {"config": "c3s", "program": f.prog_name, "socks": S, "batch": B, "packets": n,
                "rules_ipv4": w.n4, "port_rules": w.nports, "pass_frames": int(c1[2 * S]),
                "calls_per_round": {"per_socket_loop": 2 * S, "single_call": 2}}
        for k in legs:
            med = statistics.median(us[k])
            line[k] = {"us_per_round": [round(u, 1) for u in us[k]], "median_us": round(med, 1),
                       "Mpps": round(n / med, 2), "rounds_per_run": rounds[k],
                       "spread": round((max(us[k]) - min(us[k])) / med, 3), "kernel_path": paths[k]}
        line["ratio"] = round(line["per_socket_loop"]["median_us"] / line["single_call"]["median_us"], 2)
        # faster by more than the runs of either leg differ among themselves
        line["single_call_faster_beyond_spread"] = bool(max(us["single_call"]) < min(us["per_socket_loop"]))
        print(json.dumps(line), flush=True)
        for b in [d_rx, d_tx, d_fill] + d_v + d_c:
            b.free()
    f.close()


def run_c3sm(args):
    """c3m's three-record packets scattered over S sockets of B records: every
    socket's batch is packets of a head and two continuation chunks from its
    record 0 on; B is no multiple of 3, so the last record of an even socket is
    a packet of its own and that of an odd socket the head of a packet the
    batch ends in the middle of.  The round as the per-ring calls make it --
    xfg_classify_descs_frags (a host synchronisation each) and
    xfg_ring_egress(MULTIBUF) a socket -- beside one xfg_classify_socks_frags
    and one xfg_socks_frags_egress; first both are checked to produce the same
    rings.  Whole rounds by host wall clock as c3s times them, then each leg's
    classify calls and egress calls alone (the per-step split)."""
    import ctypes as C
    import statistics
    import numpy as np
    import xfgpu as G
    points = ([(s, b) for b in (64, 256) for s in (4, 64, 1024)] if args.sweep
              else [(args.socks, args.batch)])
    most = max(s * b for s, b in points)
    w = c3d_workload(args, "c3sm", umem_chunks=3, log2_default=max(12, (most - 1).bit_length()),
                     descs_min_packets=0)
    f, nf, stride = w.f, w.n, w.stride
    assert most <= nf, "more records than --log2-packets frames"
    # continuation chunk nf + k holds a frame that hits a rule (as c3m's do)
    f.classify_descs(w.d_umem.ptr, w.d_descs.ptr, nf, w.d_verd.ptr, first=w.first, mask=w.entries - 1)
    f.sync()
    hv = w.d_verd.download(np.zeros(nf, np.uint8))
    hit = np.flatnonzero(hv == 2)[:4096]          # (deny program: a hit passes)
    assert len(hit) >= 16, "no frames that hit a rule"
    which = hit[np.random.default_rng(14).integers(0, len(hit), most)]
    buf = np.zeros((most, C3D_CHUNK), np.uint8)
    buf[:, C3D_HEADROOM:C3D_HEADROOM + stride] = w.data.reshape(nf, stride)[which]
    G._check(G.lib.xfg_memcpy_h2d(f.ctx, 0, w.d_umem.ptr + nf * C3D_CHUNK, buf.ctypes.data,
                                  buf.nbytes), "memcpy_h2d")
    del buf
    CONTD = np.uint64(G.XDP_PKT_CONTD << 32)
    lib, ctx = G.lib, f.ctx
    for S, B in points:
        n, R = S * B, 2 * B                    # every ring twice the batch, wrapping inside it
        first = R - 7
        j = np.arange(B)
        s_of = np.repeat(np.arange(S), B)
        head = np.tile(j % 3 == 0, S)
        # a record continues its packet unless it is the packet's third, or an
        # even socket's last record
        cont = np.tile(j % 3 != 2, S) & ~(np.tile(j == B - 1, S) & (s_of % 2 == 0))
        nh, nc = int(head.sum()), int((~head).sum())
        rec = np.zeros((n, 2), np.uint64)
        rec[head, 0] = w.perm[:nh].astype(np.uint64) * np.uint64(C3D_CHUNK) + np.uint64(C3D_HEADROOM)
        rec[head, 1] = w.lens[:nh].astype(np.uint64)
        rec[~head, 0] = (nf + np.arange(nc)).astype(np.uint64) * np.uint64(C3D_CHUNK) + np.uint64(C3D_HEADROOM)
        rec[~head, 1] = w.lens[which[:nc]].astype(np.uint64)
        rec[cont, 1] |= CONTD
        descs = np.zeros((S, R, 2), np.uint64)
        descs[:, (first + j) & (R - 1)] = rec.reshape(S, B, 2)
        d_rx = f.alloc(descs.nbytes)
        d_rx.upload(descs)
        d_tx, d_fill = [f.alloc(16 * S * R) for _ in range(2)], [f.alloc(8 * S * R) for _ in range(2)]
        d_v = [f.alloc(n), f.alloc(n)]
        d_c = [f.alloc(16 * S), f.alloc(8 * (2 * S + 2))]
        for d in d_tx + d_fill:
            d.upload(np.zeros(d.nbytes, np.uint8))

        def rings(k):
            return [dict(rx_descs=d_rx.ptr + 16 * R * s, rx_first=first, rx_mask=R - 1,
                         tx_descs=d_tx[k].ptr + 16 * R * s, tx_first=R - 5, tx_mask=R - 1,
                         fill_addrs=d_fill[k].ptr + 8 * R * s, fill_first=R - 3, fill_mask=R - 1, count=B)
                    for s in range(S)]

        # leg 1: the structures of every call built once, the library called directly
        per = []
        for s, r in enumerate(rings(0)):
            db = G.DescBatch(w.d_umem.ptr, r["rx_descs"], first, R - 1, B)
            fr = G.Frags(C.sizeof(G.Frags), None)
            e = G.Egress(C.sizeof(G.Egress), None, r["rx_descs"], first, R - 1, r["tx_descs"],
                         r["tx_first"], R - 1, r["fill_addrs"], r["fill_first"], R - 1, 0,
                         d_c[0].ptr + 16 * s, G.EGRESS_MULTIBUF)
            per.append((C.byref(db), fr, e, d_v[0].ptr + s * B, db))
        tab = G.sock_table(rings(1))
        sk = G.Socks(C.sizeof(G.Socks), w.d_umem.ptr, tab, None, S)
        done = (C.c_uint32 * S)()
        sfr = G.SocksFrags(C.sizeof(G.SocksFrags), done, None)
        se = G.SocksEgress(C.sizeof(G.SocksEgress), None, 0, 0, d_c[1].ptr, 0)

        def loop_classify():
            for db, fr, e, v, _ in per:
                rc = lib.xfg_classify_descs_frags(ctx, 0, db, C.byref(fr), v, None)
                assert rc == 0, rc
                e.count = fr.counts[1]             # frags_done: what the egress takes

        def loop_egress():
            for _, _, e, v, _ in per:
                rc = lib.xfg_ring_egress(ctx, 0, C.byref(e), v, None)
                assert rc == 0, rc

        def loop_round():
            for db, fr, e, v, _ in per:
                rc = lib.xfg_classify_descs_frags(ctx, 0, db, C.byref(fr), v, None)
                e.count = fr.counts[1]
                rc = rc or lib.xfg_ring_egress(ctx, 0, C.byref(e), v, None)
                assert rc == 0, rc

        def single_classify():
            rc = lib.xfg_classify_socks_frags(ctx, 0, C.byref(sk), C.byref(sfr), d_v[1].ptr, None)
            assert rc == 0, rc

        def single_egress():
            rc = lib.xfg_socks_frags_egress(ctx, 0, C.byref(sk), C.byref(se), done, d_v[1].ptr, None)
            assert rc == 0, rc

        def single_round():
            single_classify()
            single_egress()

        # both legs make the same round: verdicts of the live records, done[],
        # every ring whole, every count
        loop_round()
        single_round()
        f.sync()
        want_done = np.where(np.arange(S) % 2 == 0, B, B - B % 3 if B % 3 else B)
        got_done = np.frombuffer(done, np.uint32)
        assert np.array_equal(got_done, want_done), "done[] differs"
        assert np.array_equal(got_done, [int(p[1].counts[1]) for p in per])
        assert tuple(sfr.counts) == (sum(int(p[1].counts[0]) for p in per), int(got_done.sum()),
                                     n - int(got_done.sum()))
        live = np.tile(j, S) < np.repeat(got_done.astype(np.int64), B)
        v0, v1 = (d.download(np.zeros(n, np.uint8)) for d in d_v)
        assert np.array_equal(v0[live], v1[live]) and np.all(v1[~live] == G.VERDICT_NONE)
        for pair in (d_tx, d_fill):
            r0, r1 = (d.download(np.zeros(d.nbytes, np.uint8)) for d in pair)
            assert r0.any() and np.array_equal(r0, r1), "the rings differ"
        c0 = d_c[0].download(np.zeros(2 * S, np.uint64))
        c1 = d_c[1].download(np.zeros(2 * S + 2, np.uint64))
        assert np.array_equal(c0, c1[:2 * S]) and int(c1[2 * S]) == int(np.count_nonzero(v1 == 2))
        legs = {"per_socket_loop": loop_round, "single_call": single_round}
        steps = {"per_socket_loop_classify": loop_classify, "per_socket_loop_egress": loop_egress,
                 "single_call_classify": single_classify, "single_call_egress": single_egress}
        timed = dict(legs, **steps)
        rounds, us, paths = {}, {k: [] for k in timed}, {}
        for k, one in timed.items():                # warm-up, and how many rounds a run needs
            for _ in range(3):
                one()
            f.sync()
            t0 = time.perf_counter()
            for _ in range(3):
                one()
            f.sync()
            rounds[k] = int(min(2000, max(5, 0.1 / ((time.perf_counter() - t0) / 3))))
            paths[k] = f.last_path()
        for _ in range(max(5, args.runs)):
            for k, one in timed.items():
                t0 = time.perf_counter()
                for _ in range(rounds[k]):
                    one()
                f.sync()
                us[k].append((time.perf_counter() - t0) / rounds[k] * 1e6)
        line = {"config": "c3sm", "program": f.prog_name, "socks": S, "batch": B, "records": n,
                "packets": int(sfr.counts[0]), "records_in_packets": int(sfr.counts[1]),
                "trailing_records": int(sfr.counts[2]), "rules_ipv4": w.n4, "port_rules": w.nports,
                "pass_records": int(c1[2 * S]),
                "calls_per_round": {"per_socket_loop": 2 * S, "single_call": 2},
                "host_syncs_per_round": {"per_socket_loop": S, "single_call": 1}}
        for k in legs:
            med = statistics.median(us[k])
            line[k] = {"us_per_round": [round(u, 1) for u in us[k]], "median_us": round(med, 1),
                       "Mrecords_per_s": round(n / med, 2), "rounds_per_run": rounds[k],
                       "spread": round((max(us[k]) - min(us[k])) / med, 3), "kernel_path": paths[k]}
        line["steps_median_us"] = {k: round(statistics.median(us[k]), 1) for k in steps}
        line["ratio"] = round(line["per_socket_loop"]["median_us"] / line["single_call"]["median_us"], 2)
        # faster by more than the runs of either leg differ among themselves
        line["single_call_faster_beyond_spread"] = bool(max(us["single_call"]) < min(us["per_socket_loop"]))
        print(json.dumps(line), flush=True)
        for b in [d_rx] + d_tx + d_fill + d_v + d_c:
            b.free()
    f.close()


def run(name, args):
    import numpy as np
    import xftools as X
    import xfgpu as G
    if name == "c3sm":
        return run_c3sm(args)
    if name == "c3s":
        return run_c3s(args)
    if name == "c1":
        return run_c1(args)
    if name == "c3c":
        return run_c3c(args)
    if name == "c3ch":
        return run_c3ch(args)
    if name == "c3d":
        return run_c3d(args)
    if name == "c3f":
        return run_c3f(args)
    if name == "c3st":
        return run_c3st(args)
    if name == "c3fw":
        return run_c3fw(args)
    if name == "c3m":
        return run_c3m(args)
    if name == "c3mfw":
        return run_c3mfw(args)
    if name == "c3mc":
        return run_c3mc(args)
    if name == "c3mst":
        return run_c3mst(args)
    if name == "c3mch":
        return run_c3mch(args)
    kind = {"c2": 2, "c3": 3, "c4": 4, "c5": 5, "c3sd": 3, "c3e": 3}[name]
    n = 1 << (args.log2_packets or {"c2": 24, "c3": 24, "c4": 23, "c5": 23, "c3sd": 24, "c3e": 24}[name])
    stride = 64 if kind in (2, 3) else 1536
    n4 = {2: 1000, 3: 1_000_000, 4: 1_000_000, 5: 15_000_000}[kind]
    flag = 3 if name == "c3sd" else 2
    n6 = 1_000_000 if kind == 5 else 0
    nports = 1024 if kind == 5 else 16
    t0 = time.time()
    v4 = X.rand_keys(kind, int(n4 * 1.02) + 16, 4)[:n4]
    v6 = X.rand_keys(kind + 100, int(n6 * 1.02) + 16, 16)[:n6] if n6 else None
    ports = (np.arange(nports, dtype=np.uint32) * 61 + 53).astype(np.uint16)
    print(f"[{name}] keys {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    data, lens = X.gen_workload(kind, kind, n, stride, v4=v4, v6=v6, ports=ports)
    print(f"[{name}] frames {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    feats = G.FEAT_IPV4 | G.FEAT_IPV6 | G.FEAT_DENY if kind == 2 else G.FEAT_ALL | G.FEAT_DENY
    f = G.Filter(feats, devices=[0], ipv4_capacity=n4, ipv6_capacity=max(n6, 1024))
    f.update_batch(G.MAP_IPV4, v4, np.full(len(v4), flag, np.uint64))
    if n6:
        f.update_batch(G.MAP_IPV6, v6, np.full(len(v6), 2, np.uint64))
    if kind != 2:
        pk = np.array([X.port_key(int(p)) for p in ports], "<u4").view(np.uint8)
        f.update_batch(G.MAP_PORTS, pk, np.full(len(ports), 2 | 4 | 8, np.uint64))
    if name == "c3e":   # C1's MAC rules, a ruled MAC where its rule looks in 10 % of the frames
        er = X.c1_rules().prepared()
        f.update_batch(G.MAP_ETHERNET, er.eth_keys, er.eth_vals)
        rng = np.random.default_rng(9)
        d = data.reshape(n, stride)
        pick = rng.choice(n, n // 10, replace=False)
        which = rng.integers(0, len(er.eth_keys), len(pick))
        dst = (er.eth_vals[which] & 2) != 0
        d[pick[dst], 0:6] = er.eth_keys[which[dst]]
        d[pick[~dst], 6:12] = er.eth_keys[which[~dst]]
    setup_s = time.time() - t0
    print(f"[{name}] rules loaded {setup_s:.1f}s", file=sys.stderr, flush=True)
    alg = int(np.minimum(lens.astype(np.int64), 128).sum() + n)
    d_data, d_lens, d_verd = f.alloc(data.nbytes), f.alloc(lens.nbytes), f.alloc(n)
    d_data.upload(data)
    d_lens.upload(lens)
    f.classify_timed(d_data.ptr, d_lens.ptr, n, stride, d_verd.ptr, 2)
    ms = f.classify_timed(d_data.ptr, d_lens.ptr, n, stride, d_verd.ptr, args.iters)
    line = {"config": name, "program": f.prog_name, "packets": n, "stride": stride,
            "kernel_path": f.last_path(),
            "rules_ipv4": n4, "rules_ipv6": n6, "port_rules": nports if kind != 2 else 0,
            "kernel_ms": round(ms, 4), "Mpps": round(n / (ms * 1e-3) / 1e6, 1),
            "roofline": {"alg_bytes_per_launch": alg,
                         "achieved_GBps": round(alg / (ms * 1e-3) / 1e9, 1),
                         "frac": round(alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            "setup_s": round(setup_s, 1)}
    if kind == 5 and not args.no_host:
        # end to end from host memory: whole frames and lengths H2D, verdicts D2H
        f.classify_host(data, lens, stride=stride)
        t1 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            f.classify_host(data, lens, stride=stride)
        hs = (time.perf_counter() - t1) / reps
        pcie = n * (128 + 4) + n   # header windows + lengths H2D, verdicts D2H
        line["host_path"] = {"Mpps": round(n / hs / 1e6, 2), "ms": round(hs * 1e3, 2),
                             "pcie_bytes": pcie, "GBps_pcie": round(pcie / hs / 1e9, 1),
                             "frame_GBps": round(data.nbytes / hs / 1e9, 1),
                             "note": "xfg_classify_host: 128 B header windows + u32 lens H2D "
                                     "(gathered by the per-device pool), verdicts D2H; frames "
                                     "whose program leaves the window go again whole (none "
                                     "in this mix)"}
        # the same frames registered once (a capture ring / UMEM kept by the
        # caller, xfg_host_register): the kernel reads the 64 B header
        # windows of the 1536 B slots in place over PCIe (zero copy), the
        # pool gathers the lengths only
        f.host_register(data)
        f.classify_host(data, lens, stride=stride)
        t1 = time.perf_counter()
        for _ in range(reps):
            f.classify_host(data, lens, stride=stride)
        hr = (time.perf_counter() - t1) / reps
        f.host_unregister(data)
        zpcie = n * (64 + 4) + n   # windows read in place, lengths H2D, verdicts D2H
        line["host_path"].update({"registered_Mpps": round(n / hr / 1e6, 2),
                                  "registered_ms": round(hr * 1e3, 2),
                                  "registered_pcie_bytes": zpcie,
                                  "registered_GBps_pcie": round(zpcie / hr / 1e9, 1),
                                  "registered_frame_GBps": round(data.nbytes / hr / 1e9, 1)})
    f.close()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["c2", "c4", "c5", "c3sd"])
    ap.add_argument("--log2-packets", type=int, default=0,
                    help="batch size (c3d: 22 by default, an 8 GiB UMEM of 2 KiB chunks; "
                         "the workload's 2^24 would need 32 GiB beside the other buffers)")
    ap.add_argument("--runs", type=int, default=3, help="c3d: timed runs of each leg")
    ap.add_argument("--no-cpu", action="store_true", help="c1: the GPU leg only")
    ap.add_argument("--no-host", action="store_true",
                    help="c5: the device-resident leg only (PMC passes of its kernel)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--socks", type=int, default=64, help="c3s, c3sm: sockets a round")
    ap.add_argument("--batch", type=int, default=64,
                    help="c3s, c3sm: records peeked from each socket (a power of two)")
    ap.add_argument("--sweep", action="store_true",
                    help="c3s, c3sm: sockets 4, 64, 1024 x batch 64, 256 instead of one point")
    a = ap.parse_args()
    for c in a.configs:
        run(c, a)


if __name__ == "__main__":
    main()

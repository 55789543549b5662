/* SPDX-License-Identifier: GPL-2.0 */
/*
 * xdpfilter_gpu.h — C ABI of the MI355X-native xdp-filter classifier.
 *
 * This is the drop-in boundary for xdp-filter's per-packet hot path: the ten
 * eBPF programs xdpfilt_{alw,dny}_{all,eth,ip,tcp,udp} built from
 * xdp-filter/xdpfilt_prog.h:214-310 (reference v1.6.3), their BPF maps
 * (xdp-filter/xdpfilt_prog.h:67-185, headers/xdp/xdp_stats_kern.h:20-26) and
 * the userspace operations the xdp-filter CLI performs on them
 * (xdp-filter/xdp-filter.c:48-157).  The per-packet program becomes a batch
 * HIP kernel over packets resident in HBM; the per-CPU BPF maps become
 * per-device tables whose values keep the reference encoding
 * (hits << COUNTER_SHIFT) | flags.
 *
 * Plain C types only (no HIP/torch types): streams are passed as void*
 * (a hipStream_t, or NULL for the device's default stream of this library).
 * Errors are negative errno values, as in libxdp/libbpf
 * (headers/xdp/libxdp.h:51-53).
 */
#ifndef XDPFILTER_GPU_H
#define XDPFILTER_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants: identical values to xdp-filter/common_kern_user.h:4-19 ---- */
#define XFG_FEAT_TCP      (1u << 0)
#define XFG_FEAT_UDP      (1u << 1)
#define XFG_FEAT_IPV6     (1u << 2)
#define XFG_FEAT_IPV4     (1u << 3)
#define XFG_FEAT_ETHERNET (1u << 4)
#define XFG_FEAT_ALL      (XFG_FEAT_TCP | XFG_FEAT_UDP | XFG_FEAT_IPV6 | \
			   XFG_FEAT_IPV4 | XFG_FEAT_ETHERNET)
#define XFG_FEAT_ALLOW    (1u << 5)
#define XFG_FEAT_DENY     (1u << 6)

#define XFG_MAP_FLAG_SRC  (1u << 0)
#define XFG_MAP_FLAG_DST  (1u << 1)
#define XFG_MAP_FLAG_TCP  (1u << 2)
#define XFG_MAP_FLAG_UDP  (1u << 3)
#define XFG_MAP_FLAGS     (XFG_MAP_FLAG_SRC | XFG_MAP_FLAG_DST | \
			   XFG_MAP_FLAG_TCP | XFG_MAP_FLAG_UDP)
#define XFG_COUNTER_SHIFT 6

/* enum xdp_action values (headers/linux/bpf.h:6130-6136) */
#define XFG_XDP_ABORTED   0
#define XFG_XDP_DROP      1
#define XFG_XDP_PASS      2
#define XFG_ACTION_MAX    5   /* XDP_REDIRECT + 1, headers/xdp/xdp_stats_kern_user.h:21 */

/* Default hash-map capacity = the reference's max_entries
 * (xdp-filter/xdpfilt_prog.h:115,146,181). */
#define XFG_DEFAULT_MAP_CAPACITY 10000u
#define XFG_PORT_MAP_ENTRIES     65536u   /* xdp-filter/xdpfilt_prog.h:69 */

/* Maps, named as the reference pins them (xdp-filter/common_kern_user.h:21-24). */
enum xfg_map_id {
	XFG_MAP_PORTS    = 0, /* "filter_ports":    key u32 = raw be16 port (htons(port)), PERCPU_ARRAY */
	XFG_MAP_IPV4     = 1, /* "filter_ipv4":     key 4 bytes, network order */
	XFG_MAP_IPV6     = 2, /* "filter_ipv6":     key 16 bytes (struct in6_addr) */
	XFG_MAP_ETHERNET = 3, /* "filter_ethernet": key 6 bytes (struct ethaddr) */
	XFG_MAP_NUM      = 4,
};

/* struct xdp_stats_record, headers/xdp/xdp_stats_kern_user.h:10-19 */
struct xfg_stats_record {
	uint64_t packets;
	uint64_t bytes;
};

typedef struct xfg_ctx xfg_ctx;

struct xfg_open_opts {
	size_t sz;               /* sizeof(struct xfg_open_opts), for extension */
	uint32_t features;       /* XFG_FEAT_* requested | XFG_FEAT_ALLOW or _DENY */
	const int *devices;      /* HIP device ordinals; NULL with ndev>0 => 0..ndev-1 */
	int ndev;                /* 0 => host-only context: map CRUD works, classify -ENODEV */
	uint32_t ipv4_capacity;  /* 0 => XFG_DEFAULT_MAP_CAPACITY */
	uint32_t ipv6_capacity;
	uint32_t eth_capacity;
	uint32_t hash_seed;      /* 0 => fixed default seed */
	/* IPv4 maps with at least this many keys are looked up through the
	 * one-read quotient index when it applies (fixed-stride batches, no
	 * live Ethernet key, one or both IPv4 lookup directions live, the same
	 * flags on every device): 0 =>
	 * default (2^18), UINT32_MAX => never.  Results never depend on it. */
	uint32_t qt_min_keys;
	/* Header window of the pipelined kernels for fixed-stride batches
	 * whose stride exceeds 64 bytes: 0 => 64 (default: half the bytes of
	 * a 128-byte window per frame; a frame whose parse reaches past byte
	 * 64 -- IPv6/TCP, long IPv6 extension chains, IPv4 options -- takes the
	 * deferred walk over the whole frame), 128 => 128-byte windows.
	 * Results never depend on it.  AF_XDP descriptor batches on the
	 * pipelined kernel use the same window. */
	uint32_t window;
	uint32_t reserved0;      /* (the earlier layout's tail padding: ignored) */
	/* AF_XDP descriptor batches (xfg_classify_descs) of at least this many
	 * packets take the pipelined kernel, smaller ones the general kernel,
	 * whose fixed cost per launch is lower: 0 => default (2^16), 1 => every
	 * batch.  Results never depend on it. */
	uint32_t descs_min_packets;
};

/*
 * Program selection, same rule as find_prog_file() (xdp-filter/xdp-filter.c:48-60):
 * the first program in xdp-filter/Makefile:3-6 order whose feature bits are a
 * superset of @features.  Returns 0 and the program's name/features, or
 * -ENOENT (no program matches, e.g. ALLOW|DENY both set) / -EINVAL (0).
 */
int xfg_select_program(uint32_t features, const char **prog_name,
		       uint32_t *prog_features);

/* Open a context: selects the program, allocates the tables on every device. */
int xfg_open(xfg_ctx **out, const struct xfg_open_opts *opts);
void xfg_close(xfg_ctx *ctx);

const char *xfg_prog_name(const xfg_ctx *ctx);      /* e.g. "xdpfilt_dny_all" */
uint32_t xfg_prog_features(const xfg_ctx *ctx);     /* the program's _features word */
int xfg_num_devices(const xfg_ctx *ctx);            /* analogue of libbpf_num_possible_cpus() */
const char *xfg_strerror(int err);

/* The classify kernel the last launch on device @dev ran (introspection for
 * tests and tools): XFG_PATH_GENERAL (offsets, header windows, the
 * descriptor batches of the Ethernet-only programs, those below
 * xfg_open_opts.descs_min_packets and those of 2^32 packets or more),
 * _PIPELINE (fixed stride with any live key; AF_XDP
 * descriptors, xfg_classify_descs), _IPV4 (IPv4 keys only:
 * prefilter + bucket line), _QT (IPv4 keys only: the quotient index),
 * _ETH (the Ethernet-only programs, their map as an LDS key table); or
 * -EINVAL / -ENOENT (no launch yet). */
#define XFG_PATH_GENERAL  0
#define XFG_PATH_PIPELINE 1
#define XFG_PATH_IPV4     2
#define XFG_PATH_QT       5
#define XFG_PATH_ETH      6
int xfg_last_path(const xfg_ctx *ctx, int dev);

/*
 * Map operations.  As with a BPF per-CPU map, a value is one u64 per device
 * (vals[xfg_num_devices()]), or exactly one u64 on a host-only context.
 *   lookup:  -ENOENT if the key is absent (hash maps); ports always exist.
 *   update:  insert or overwrite; -E2BIG when a hash map is full.
 *   delete:  -ENOENT if absent; ports: -EINVAL (array maps cannot delete).
 *   get_next_key: key==NULL => first key; -ENOENT after the last one.
 * Key sizes: ports 4 (u32, < 65536), ipv4 4, ipv6 16, ethernet 6.
 * A value read after a classify includes every hit of the classifies queued
 * before it on that device (the quotient-index path keeps its counts per
 * index slot on the device; the first IPv4-map read, write or all-reduce
 * after it folds them in, one kernel on the device's stream).
 */
int xfg_map_lookup(xfg_ctx *ctx, int map, const void *key, uint64_t *vals);
int xfg_map_update(xfg_ctx *ctx, int map, const void *key, const uint64_t *vals);
int xfg_map_delete(xfg_ctx *ctx, int map, const void *key);
int xfg_map_get_next_key(xfg_ctx *ctx, int map, const void *key, void *next_key);
/* Bulk insert/overwrite with per-device values, as bpf_map_update_elem()
 * takes one value per possible CPU: vals[i * nvals + d] is device d's value
 * of key i (nvals = max(xfg_num_devices(), 1)).  The rule store reloads
 * saved hit counts onto one device with it (xdpfilter_io.h). */
int xfg_map_update_batch_percpu(xfg_ctx *ctx, int map, const void *keys,
				const uint64_t *vals, uint64_t n);
/* Number of keys present (ports: number of non-zero entries). */
int64_t xfg_map_count(xfg_ctx *ctx, int map);
/* Bulk lookup of @n keys (status readout, parity checks): vals[i*ndev + d]
 * receives device d's value of key i, present[i] (if not NULL) 1/0; absent
 * keys read as 0.  Returns the number of keys found or a negative errno. */
int64_t xfg_map_lookup_batch(xfg_ctx *ctx, int map, const void *keys, uint64_t n,
			     uint64_t *vals, uint8_t *present);
/* Bulk insert/overwrite of @n keys with the same value on every device
 * (rule-set loading).  Returns 0 or the first error (-E2BIG, ...). */
int xfg_map_update_batch(xfg_ctx *ctx, int map, const void *keys, const uint64_t *vals,
			 uint64_t n);

/*
 * A packet batch resident on ONE device.  Packet i starts at
 *   data + (offsets ? offsets[i] : i * stride)
 * and is lens[i] bytes long (u16 lens if lens_u16, else u32).  Every packet
 * start must be 16-byte aligned and the buffer readable up to the next
 * 16-byte boundary past its end (AF_XDP UMEM chunks and the pcap/synthetic
 * ingest paths of this library satisfy this).  Packet length is not limited
 * by stride when offsets are given.
 */
struct xfg_batch {
	const void *data;
	const uint64_t *offsets;
	const void *lens;
	uint64_t count;
	uint32_t stride;
	uint32_t lens_u16;
};

/*
 * Classify a device-resident batch on device @dev (index into the context's
 * devices): writes one enum xdp_action byte per packet to @verdicts (device
 * memory), bumps the matched rule's counter on that device and records
 * per-action stats, exactly as xdpfilt_<mode>() + xdp_stats_record_action()
 * do per packet.  Stream-ordered on @stream (hipStream_t or NULL).
 */
int xfg_classify(xfg_ctx *ctx, int dev, const struct xfg_batch *batch,
		 uint8_t *verdicts, void *stream);

/*
 * AF_XDP descriptors in device memory: packet i is RX ring
 * record descs[(first + i) & mask], a struct xdp_desc {u64 addr; u32 len;
 * u32 options} (headers/linux/if_xdp.h:110-114, read with
 * xsk_ring_cons__rx_desc(), headers/xdp/xsk.h:79-85), over the UMEM at
 * @umem: its bytes start at umem + (addr & ((1 << 48) - 1)) + (addr >> 48)
 * (xsk_umem__add_offset_to_addr(), headers/xdp/xsk.h:173-186) and it is len
 * bytes long.  mask = ring entries - 1 (a power of two), or 0xffffffff for
 * a plain array.  Frame starts must be 16-byte aligned (default UMEM frame
 * sizes and headroom are) and readable up to the next 16-byte boundary past
 * their end.  Every record is taken as a whole packet (XDP_PKT_CONTD is not
 * looked at): the batches of a socket bound with XDP_USE_SG, whose packets may
 * span several records, go through xfg_classify_descs_frags.
 */
struct xfg_desc_batch {
	const void *umem;
	const void *descs;
	uint32_t first;
	uint32_t mask;
	uint64_t count;
};

int xfg_classify_descs(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
		       uint8_t *verdicts, void *stream);

/*
 * Multi-buffer AF_XDP packets (a socket bound with XDP_USE_SG delivers a frame
 * longer than its chunk, or an LRO/GRO aggregate, as several RX records):
 * classify by the head record, one verdict byte per record.
 *
 * Packets, as l2fwd() and rx_drop() take them (lib/util/xdpsock.c:70,
 * 1228-1257,1500-1548): a packet is a maximal run of consecutive records of
 * @batch ending at the first one whose options & XFG_XDP_PKT_CONTD is 0
 * (IS_EOP_DESC); other option bits are ignored.  Record 0 starts a packet: the
 * caller released exactly counts[1] records after the previous batch, as
 * l2fwd releases frags_done.
 *
 * An XDP program sees the first buffer only (ctx->data .. ctx->data_end is the
 * head fragment), so a packet's verdict, rule hit and stats are those of the
 * program run on its head record alone, with len the head's len: rx_bytes
 * counts the head's bytes, not the packet's (headers/xdp/xdp_stats_kern.h:
 * 44-45).  Continuation records are never parsed and bump no counter and no
 * statistic.  A packet the batch ends in the middle of is not processed at
 * all -- no verdict, no stats; the caller leaves its records on the ring for
 * the next batch (lib/util/xdpsock.c:1539-1542).
 *
 * Out: counts[0] = complete packets, counts[1] = the records in them
 * (l2fwd's frags_done: what to release, and the count of the egress call),
 * counts[2] = the records of the trailing incomplete packet; counts[1] +
 * counts[2] == count.  counts is HOST memory, valid when the call returns.
 * verdicts (device, count bytes): every record of a complete packet gets its
 * packet's verdict, so xfg_ring_egress (with XFG_EGRESS_MULTIBUF) and
 * xfg_capture_descs keep their per-record interface; bytes at indices >=
 * counts[1] are not written.  pkt_of (device, count x u32, or NULL): record
 * i's packet index, the number of end-of-packet records before it, written
 * for all count records; the value counts[0] marks the trailing incomplete
 * packet.
 *
 * Three steps on the device: a head pass over the records (one kernel: the
 * packet indices, the head records gathered into a plain descriptor array in
 * library scratch, the counts); the counts read back to the host; the
 * counts[0] heads classified as xfg_classify_descs classifies a plain array
 * of that many records -- xfg_last_path and xfg_open_opts.descs_min_packets
 * behave as for such a call -- and their verdicts spread over the records.
 * The read-back is the call's one host synchronisation, after it has ordered
 * itself behind @stream, and it is deliberate: the classify launch is planned
 * on the host from the packet count (kernel, grid, the descs_min_packets
 * threshold; xfg_plan.c), and the caller needs counts[1] on the host for
 * xsk_ring_cons__release anyway.  (Classifying all count records with no-op
 * entries for the continuations would run the program on things that are not
 * packets and need the ABORTED statistic repaired afterwards.)  The classify
 * and the spread are stream-ordered; the call returns without waiting for
 * them, and @stream's later work runs after them.
 *
 * -EINVAL: what xfg_classify_descs refuses, fr == NULL, sz below the
 * structure's size, pkt_of not 4-byte aligned, count >= 2^32.  -ENODEV on a
 * host-only context.  count == 0: three zero counts, nothing launched.  No
 * end-of-packet record in the batch: {0, 0, count}, nothing classified, no
 * stats change, verdicts untouched.
 *
 * Capture by whole packet: xfg_capture_descs_frags with count = counts[1]
 * (xfg_capture_descs keeps capturing record by record, each record's bytes
 * under its packet's verdict).  A second context on the packets this one
 * passed on: xfg_classify_descs_frags_chain with count = counts[1].  Not
 * covered: xfg_classify_xsk_host, and the CLI.
 */
#define XFG_XDP_PKT_CONTD (1u << 0)          /* headers/linux/if_xdp.h:123 */

struct xfg_frags {
	size_t sz;            /* sizeof(struct xfg_frags), for extension */
	uint32_t *pkt_of;     /* device, count x u32, or NULL: record i's packet index */
	uint64_t counts[3];   /* HOST, out: packets, records in them (l2fwd's frags_done),
	                       * records of the trailing incomplete packet */
};

int xfg_classify_descs_frags(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
			     struct xfg_frags *fr, uint8_t *verdicts, void *stream);

/*
 * Chained contexts: run this context's program only on the frames an earlier
 * stage passed on.  xdp-filter is never the last word on a packet: it chains
 * on XDP_PASS (xdp-filter/xdpfilt_prog.h:209-212), and the dispatcher runs the
 * next program only on a frame whose return value is in the previous
 * program's chain_call_actions (lib/libxdp/xdp-dispatcher.c.in:59-79: if
 * (!((1U << ret) & conf.chain_call_actions[i])) return ret;).  Two stages
 * express what one program cannot, e.g. an allow-list context for ports
 * followed by a deny-list context for addresses.
 *
 * @verdicts (device, count bytes) is input and output: what an earlier stage
 * wrote for the same batch -- another context, or this one.  Frame i is
 * selected if its byte v = verdicts[i] is below 32 and bit v of chain_mask is
 * set (xfg_capture's rule for its action_mask); XFG_VERDICT_NONE and every
 * other byte >= 32 is never selected.  The verdicts, rule hit counts and
 * per-action statistics of THIS context are exactly those of running its
 * program on the selected frames alone, in their order.  A selected frame's
 * byte is replaced by the new verdict; every other byte of @verdicts is left
 * as it was.  The earlier stage's context is not touched: as in the
 * dispatcher, each program keeps its own statistics.
 *
 * Out: counts[0] = frames selected, counts[1] = frames not selected
 * (counts[0] + counts[1] == count); HOST memory, valid when the call returns.
 * idx (device, count x u32, or NULL): the selected frames' indices, ascending,
 * counts[0] of them.
 *
 * Three steps on the device, as for xfg_classify_descs_frags: a select pass
 * over the verdict bytes (one kernel: idx and the selected frames as a plain
 * descriptor array in library scratch -- a descriptor batch's records as
 * received; a struct xfg_batch's frames as {addr = the byte offset from data,
 * i * stride or offsets[i]; len = min(lens[i], stride) for a fixed stride,
 * else lens[i]; options = 0}); the selected count read back to the host; the
 * counts[0] descriptors classified as xfg_classify_descs classifies a plain
 * array of that many records over umem (or data) -- xfg_last_path and
 * xfg_open_opts.descs_min_packets behave as for such a call -- and their
 * verdicts scattered to verdicts[idx[k]].  So a fixed-stride batch chained
 * this way runs the descriptor kernels (the generic pipelined kernel, or the
 * general one), not the quotient-index loop of xfg_classify.  The read-back is
 * the call's one host synchronisation, after it has ordered itself behind
 * @stream, and deliberate for the reason given at xfg_classify_descs_frags:
 * the classify launch is planned on the host from the frame count.  The
 * classify and the scatter are stream-ordered; the call returns without
 * waiting for them, and @stream's later work runs after them.
 *
 * -EINVAL: what the matching unchained call refuses, ch == NULL, sz below the
 * structure's size, a non-zero flags, idx not 4-byte aligned, verdicts == NULL
 * with count != 0, count >= 2^32, a fixed-stride batch of more than 2^48 bytes.
 * count == 0: counts {0, 0}, nothing launched, whatever the context's devices.
 * -ENODEV on a host-only context, after these checks; no device pointer is
 * touched before it.  chain_mask == 0 or no frame selected: counts {0, count},
 * nothing classified, no statistic changes, verdicts untouched.
 *
 * Unchecked precondition: with offsets, every offset is below 2^48 -- it
 * travels in a descriptor's address field, and the device cannot refuse it.
 *
 * Many sockets need nothing of their own: with xfg_socks.flat given,
 * xfg_classify_socks leaves a plain descriptor array, and
 * xfg_classify_descs_chain takes it.  Multi-buffer batches (XDP_USE_SG
 * sockets) take xfg_classify_descs_frags_chain below: xfg_classify_descs_chain
 * would run the program on continuation records, which are not packets.  Not
 * covered: the host-memory path, and the CLI.
 */
#define XFG_CHAIN_PASS (1u << XFG_XDP_PASS)   /* xdp-filter's own chain_call_actions */

struct xfg_chain {
	size_t sz;            /* sizeof(struct xfg_chain), for extension */
	uint32_t chain_mask;  /* bit v: a frame whose verdict byte is v (< 32) runs this context's program */
	uint32_t flags;       /* 0; any bit set: -EINVAL */
	uint32_t *idx;        /* device, count x u32, 4-byte aligned, or NULL (library scratch):
	                       * out, the selected frames' indices, ascending */
	uint64_t counts[2];   /* HOST, out: frames selected, frames not selected */
};

int xfg_classify_chain(xfg_ctx *ctx, int dev, const struct xfg_batch *batch,
		       struct xfg_chain *ch, uint8_t *verdicts, void *stream);
int xfg_classify_descs_chain(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
			     struct xfg_chain *ch, uint8_t *verdicts, void *stream);

/*
 * A chained stage over a multi-buffer batch: run this context's program only
 * on the packets an earlier multi-buffer stage passed on, by their head
 * records, and give every record of such a packet the new verdict.
 *
 * @verdicts (device, count bytes) is input and output: what
 * xfg_classify_descs_frags or xfg_classify_socks_frags -- on another context,
 * or this one -- wrote for the same records.  Packets are formed exactly as
 * xfg_capture_descs_frags forms them (live / eop / head, stated there), so the
 * call serves both: after xfg_classify_descs_frags pass count = counts[1];
 * after xfg_classify_socks_frags pass sk->flat as a plain array (mask
 * 0xffffffff) of count = total records, whose XFG_VERDICT_NONE bytes keep the
 * sockets apart.  The packet of head h is records h..e; it exists only if every
 * one of them is live and e < count.  A complete packet is selected by its
 * head's byte alone: v[h] < 32 and bit v[h] of chain_mask set.  A live run that
 * ends -- at a record that is not live, or at the end of the batch -- without
 * an end-of-packet record is no packet and is never selected.
 *
 * The verdicts, rule hit counts and per-action statistics of THIS context are
 * exactly those of xfg_classify_descs over the plain array of the selected
 * packets' head records, in their order, each with its head record's len;
 * xfg_last_path and xfg_open_opts.descs_min_packets behave as for such a call
 * of counts[0] records.  The earlier stage's context is not touched.  Every
 * record h..e of a selected packet gets the new verdict byte; every other byte
 * of @verdicts stays as it was, XFG_VERDICT_NONE bytes and the bytes around an
 * unaligned @verdicts included.  So xfg_ring_egress (XFG_EGRESS_MULTIBUF),
 * xfg_socks_frags_egress and xfg_capture_descs_frags take the result as they
 * take the earlier stage's.  If every record is an end-of-packet record and no
 * byte is XFG_VERDICT_NONE, then idx, counts[0] and the verdict bytes are
 * those of xfg_classify_descs_chain.
 *
 * Out: counts[0] = packets selected, counts[1] = records in them, counts[2] =
 * all other records (count - counts[1]); HOST memory, valid when the call
 * returns.  idx (device, count x u32, or NULL): the selected packets' head
 * record indices, ascending, counts[0] of them.
 *
 * Three steps on the device, as for xfg_classify_descs_chain: the pre-pass
 * (two kernels whatever the packets' shapes: a scan over the records that
 * numbers the runs between packet boundaries, then a scan over those runs that
 * ranks the selected complete ones and gathers their head records into a plain
 * descriptor array in library scratch); the two counts read back to the host;
 * the counts[0] heads classified, and their verdicts spread over the records
 * (one kernel).  No record walks its packet: a packet of thousands of records
 * costs what that many single records cost.  16 bytes a record of library
 * scratch beside the frags calls', grown on demand.  The read-back is the
 * call's one host synchronisation, after it has ordered itself behind @stream,
 * deliberate for the reason given at xfg_classify_descs_frags.  The classify
 * and the spread are stream-ordered; the call returns without waiting for
 * them, and @stream's later work runs after them.
 *
 * -EINVAL: what xfg_classify_descs_chain refuses, of this structure: ch ==
 * NULL, sz below the structure's size, a non-zero flags, idx not 4-byte
 * aligned, verdicts == NULL with count != 0, count >= 2^32, and what
 * xfg_classify_descs refuses of the batch.  count == 0: counts {0, 0, 0},
 * nothing launched, whatever the context's devices.  -ENODEV on a host-only
 * context, after these checks; no device pointer is touched before it.
 * chain_mask == 0 or no packet selected: counts {0, 0, count}, nothing
 * classified, no statistic changes, verdicts untouched.  -EIO if a count read
 * back is impossible.  Not covered: the host-memory ring
 * (xfg_classify_xsk_host), and the CLI.
 */
struct xfg_frags_chain {
	size_t sz;            /* sizeof(struct xfg_frags_chain), for extension */
	uint32_t chain_mask;  /* bit v: a packet whose HEAD's verdict byte is v (< 32) runs this context's program */
	uint32_t flags;       /* 0; any bit set: -EINVAL */
	uint32_t *idx;        /* device, count x u32, 4-byte aligned, or NULL (library scratch):
	                       * out, the selected packets' head record indices, ascending */
	uint64_t counts[3];   /* HOST, out: packets selected, records in them,
	                       * all other records (count - counts[1]) */
};

int xfg_classify_descs_frags_chain(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
				   struct xfg_frags_chain *ch, uint8_t *verdicts, void *stream);

/*
 * Host-resident batch (struct xfg_batch in host memory): classifies it on
 * device @dev and writes the verdicts to host memory.  Only each frame's
 * first 128 bytes (its header window) and its length cross PCIe -- gathered
 * into pinned staging by a per-device thread pool and pipelined H2D / kernel
 * / D2H over chunks; a frame whose program reads past its window is sent
 * again whole and classified from it, so verdicts, counters and stats are
 * exactly those of a whole-frame run.  A fixed stride of at most 128 bytes
 * is staged slot for slot; a batch in a registered buffer
 * (xfg_host_register) is read in place instead.  Concurrent calls on different devices run in
 * parallel; staging memory per device is fixed (about 70 MB pinned).
 * Replaces the per-packet program run of the attach path
 * (xdp-filter/xdpfilt_prog.h:214-310 over frames the kernel hands it).
 */
int xfg_classify_host(xfg_ctx *ctx, int dev, const struct xfg_batch *batch,
		      uint8_t *verdicts);

/*
 * Register a long-lived host buffer (a capture ring, an AF_XDP UMEM) for
 * zero-copy reads: a host batch whose fixed-stride slots (stride a multiple
 * of 16) lie inside a registered buffer, or an AF_XDP batch
 * (xfg_classify_xsk_host) whose UMEM does, is read by the kernels where it
 * lies through the buffer's device mapping -- only the bytes the programs
 * load cross PCIe, and no frame is staged.  Pins and maps the pages
 * (hipHostRegister, portable + mapped) until xfg_host_unregister() or
 * xfg_close().  At most 16 buffers per context; -EEXIST if it overlaps a
 * registered one.
 */
int xfg_host_register(xfg_ctx *ctx, void *p, size_t bytes);
int xfg_host_unregister(xfg_ctx *ctx, void *p);

/* Threads of a device's host-path gather pool (1-16): the process's CPU set,
 * or XFG_HOST_THREADS, or OMP_NUM_THREADS when above 1 (torchrun's default
 * of 1 is not taken as the process's share).  Performance only. */
int xfg_host_threads(void);

/*
 * AF_XDP RX in host memory: the consumer side of an XDP socket's RX ring
 * (xsk_ring_cons__peek() / xsk_ring_cons__rx_desc() / xsk_ring_cons__release(),
 * headers/xdp/xsk.h:80-86,143-165).  Packet i is ring record
 * descs[(first + i) & mask], a struct xdp_desc {u64 addr; u32 len; u32
 * options} (headers/linux/if_xdp.h:110-114), over the host UMEM @umem of
 * @umem_bytes: its bytes start at umem + (addr & ((1 << 48) - 1)) +
 * (addr >> 48) (xsk_umem__add_offset_to_addr(), headers/xdp/xsk.h:173-186;
 * unaligned-chunk mode).  mask = ring entries - 1 (a power of two), or
 * 0xffffffff for a plain array; count <= entries.  Classified as
 * xfg_classify_host does (header windows, exact whole-frame fallback; a
 * registered UMEM read in place); -EINVAL if a frame lies outside the UMEM.  The caller releases the ring
 * entries after the call returns.
 */
int xfg_classify_xsk_host(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
			  uint64_t umem_bytes, uint8_t *verdicts);

/*
 * Verdict compaction: writes the indices i (ascending) with verdicts[i] ==
 * @action to @idx and their number to *@count — the list a forwarding stage
 * walks (the reference passes XDP_PASS frames on up the chain,
 * xdp-filter/xdpfilt_prog.h:209-212).  Device memory: @verdicts (n bytes),
 * @idx (room for n u32), @count (one u64).  One pass (wave ballots and
 * prefix sums, decoupled look-back between tiles), stream-ordered on @stream
 * (NULL: the library's stream of the device).  n < 2^32.
 */
int xfg_compact(xfg_ctx *ctx, int dev, const uint8_t *verdicts, uint64_t n, uint32_t action,
		uint32_t *idx, uint64_t *count, void *stream);

/*
 * AF_XDP egress: the TX and fill ring records of a classified RX batch, built
 * on the device -- what an AF_XDP consumer does with a received batch, per
 * packet by its verdict.  Packet i is RX record rx_descs[(rx_first + i) &
 * rx_mask], a struct xdp_desc as for xfg_classify_descs, and @verdicts holds
 * its verdict byte (device memory, count bytes).
 *
 * The k-th packet in packet order whose verdict is XFG_XDP_PASS becomes TX
 * record tx_descs[(tx_first + k) & tx_mask]: addr as received (the
 * unaligned-chunk form, offset in bits 48..63, stays), len as received,
 * options 0 -- l2fwd()'s tx_desc->addr = orig; tx_desc->len = len
 * (lib/util/xdpsock.c:1466-1550).  The j-th packet with any other verdict
 * byte hands its chunk back: fill_addrs[(fill_first + j) & fill_mask] = addr &
 * ((1 << 48) - 1), rx_drop()'s *xsk_ring_prod__fill_addr(fq, idx_fq++) =
 * xsk_umem__extract_addr(addr) (lib/util/xdpsock.c:1199-1258,
 * headers/xdp/xsk.h:173-176).  counts[0] = TX records, counts[1] = fill
 * addresses (device memory, two u64): the caller submits that many entries
 * of each ring; entries past them are not written.  Peek, reserve, submit
 * and release stay with the caller.
 *
 * tx_descs == NULL: every chunk goes to the fill ring (rx_drop); @verdicts is
 * not read and may be NULL.  fill_addrs == NULL: only the TX ring is written;
 * counts[1] still counts the other frames.  Both NULL: -EINVAL.
 *
 * XFG_EGRESS_SWAP_MACS: bytes 0..5 and 6..11 of every PASS frame change
 * places in the UMEM (swap_mac_addresses(), lib/util/xdpsock.c:646-654), by
 * one 16-byte load and store of the frame's first 16 bytes: frame starts are
 * 16-byte aligned as for xfg_classify_descs, and a PASS frame is at least 14
 * bytes long (every program aborts a shorter one).  With this flag the
 * descriptors of one batch must name distinct frames (two records of one
 * frame would race on its bytes).
 *
 * A mask is ring entries - 1 (a power of two), or 0xffffffff for a plain
 * array; an index first + i wraps modulo 2^32 before the mask.  The caller
 * reserves count entries of each output ring (as xsk_ring_prod__reserve(..,
 * rcvd, ..) does), so a ring of fewer entries is refused.  The TX and fill
 * rings must not overlap the RX ring or each other (not checked).
 *
 * -EINVAL: sz below the structure's size, a mask that is not 2^k - 1, an
 * output ring of fewer than count entries, a pointer that is not 8-byte
 * aligned, count >= 2^32, counts == NULL, unknown flag bits, SWAP_MACS
 * without umem, no RX ring or no verdicts where they are read.  -ENODEV on a
 * host-only context.  count == 0 writes two zero counts and nothing else.
 *
 * Stream-ordered on @stream (NULL: the library's stream of the device), as
 * xfg_compact is: after xfg_classify_descs on the same stream it needs no
 * host synchronisation.
 *
 * XFG_EGRESS_MULTIBUF: the batch holds multi-buffer packets classified by
 * xfg_classify_descs_frags -- count = its counts[1], @verdicts its per-record
 * verdicts.  A TX record's options is then the RX record's options &
 * XFG_XDP_PKT_CONTD instead of 0 (tx_desc->options = eop ? 0 : XDP_PKT_CONTD,
 * lib/util/xdpsock.c:1528), and XFG_EGRESS_SWAP_MACS touches head records
 * only (lib/util/xdpsock.c:1521-1522): record 0, and record i iff record
 * i - 1 has the bit clear.  All records of a packet carry one verdict, so the
 * order-preserving partition keeps a PASS packet's records adjacent and in
 * order on the TX ring and hands every chunk of any other packet to the fill
 * ring (rx_drop, lib/util/xdpsock.c:1248); counts stay per record, as
 * l2fwd's tx_frags is.  Without the flag every record is a packet of its own
 * (single-buffer descriptors, options 0 in the TX records).  The flag is bit
 * 2: bit 1 stays an unknown flag, refused as before.
 */
#define XFG_EGRESS_SWAP_MACS (1u << 0)
#define XFG_EGRESS_MULTIBUF  (1u << 2)

struct xfg_egress {
	size_t sz;              /* sizeof(struct xfg_egress), for extension */
	void *umem;             /* written only with SWAP_MACS; else may be NULL */
	const void *rx_descs;
	uint32_t rx_first, rx_mask;
	void *tx_descs;         /* NULL: all frames to the fill ring */
	uint32_t tx_first, tx_mask;
	uint64_t *fill_addrs;   /* NULL: TX ring only */
	uint32_t fill_first, fill_mask;
	uint64_t count;         /* < 2^32 */
	uint64_t *counts;       /* device memory, 2 x u64 */
	uint32_t flags;
};

int xfg_ring_egress(xfg_ctx *ctx, int dev, const struct xfg_egress *e,
		    const uint8_t *verdicts, void *stream);

/*
 * Steered egress: the passed frames of a classified RX batch spread over the
 * TX rings of K workers by flow, on the device -- "drop the attack, spread the
 * rest".  Worker q owns TX ring q; a flow always takes the same ring, in
 * arrival order.  This is xdp-bench redirect-cpu's cpumap_l4_hash,
 * cpumap_l4_sport and cpumap_l4_dport (xdp-bench/xdp_redirect_cpumap.bpf.c:
 * 506-653) with a TX ring in the place of a CPU.
 *
 * Record i is rx_descs[(rx_first + i) & rx_mask] with verdict byte
 * verdicts[i], as for xfg_ring_egress.  A record whose verdict is
 * XFG_XDP_PASS gets a queue, chosen from the frame's bytes [0, len) in the
 * UMEM exactly as the program chooses from [data, data_end):
 *
 *   parse_eth (:53-96): a frame with len < 14, with an ethertype below 0x0600,
 *   or whose first or second 802.1Q/802.1AD tag does not fit in the frame is
 *   refused.  At most two tags are skipped; a third leaves a VLAN ethertype,
 *   which is neither IPv4 nor IPv6.  A refused frame goes to queue skip_queue
 *   (the program returns XDP_PASS for it, "just skip": here the caller's
 *   slow-path worker) and is counted in counts[nqueues + 1].  With l3 the
 *   offset behind the tags:
 *
 *   XFG_STEER_L4_HASH (:469-553): IPv4 -- l3 + 20 > len: hash 0; else
 *   SuperFastHash (xdp-bench/hash_func01.h) of the four bytes of saddr + daddr
 *   with initial value 15485863 + protocol, the addresses loaded as the
 *   program loads them (little-endian 32-bit loads of network-order bytes,
 *   wrapping sum; swapping source and destination gives the same hash).  IPv6
 *   -- l3 + 40 > len: hash 0; else the same over the wrapping sum of the eight
 *   address words, with 15485863 + nexthdr.  ARP and everything else: hash 0.
 *   idx = hash % navail.
 *
 *   XFG_STEER_L4_SPORT / XFG_STEER_L4_DPORT (:98-213,567-641): the port, in
 *   host order, read at the fixed offset l3 + 20 (IPv4) or l3 + 40 (IPv6) --
 *   the program looks neither at ihl nor at extension headers (:111,134), so
 *   neither does this.  It is 0 unless the protocol (IPv4) or nexthdr (IPv6)
 *   is TCP and a 20-byte TCP header fits in the frame, or UDP and an 8-byte
 *   UDP header fits.  idx = port % navail.
 *
 *   queue = avail[idx] (the program's cpus_available, navail its cpus_count:
 *   a queue named twice gets twice the share).  avail == NULL: the identity,
 *   navail = nqueues.
 *
 * The k-th record in batch order that takes queue q becomes
 * queues[q].tx_descs[(tx_first + k) & tx_mask] of that queue: addr and len as
 * received, options 0.  The j-th record with any other verdict hands its chunk
 * back: fill_addrs[(fill_first + j) & fill_mask] = addr & ((1 << 48) - 1);
 * fill_addrs == NULL: no fill entries are written.  counts (device, (nqueues +
 * 2) x u64): counts[q] the TX records of queue q, counts[nqueues] the other
 * records (whether their fill entries were written or not), counts[nqueues +
 * 1] the refused frames (they are among counts[skip_queue] too).  Ring entries
 * past those counts are not written.  queue_of[i] (device, count bytes), when
 * given, is record i's queue, or XFG_QUEUE_NONE for a record that is not PASS.
 *
 * queues and avail are HOST memory and may be reused as soon as the call
 * returns: they reach the device through the pinned staging slots of the
 * socket calls, so the call makes no host synchronisation, and after
 * xfg_classify_descs on the same stream it needs none.  A queue with tx_descs
 * == NULL is refused if an avail entry or skip_queue names it.
 *
 * XFG_EGRESS_SWAP_MACS, masks, index wrap, ring overlap and stream ordering
 * are as for xfg_ring_egress; every TX ring that can be written and the fill
 * ring need at least count entries.  The UMEM is read for every PASS frame:
 * the first 64 bytes that lie below len rounded up to 16 (frame starts are
 * 16-byte aligned), and four bytes at 64 for a double-tagged IPv6 frame in
 * XFG_STEER_L4_DPORT whose port counts.  count == 0: the counts are zeroed and
 * nothing else is written.
 *
 * The call takes one RX ring or plain array.  For a poll round of many
 * sockets it runs over the flat array xfg_classify_socks leaves, with mask
 * 0xffffffff.
 *
 * -EINVAL: s == NULL, sz below the structure's size, nqueues 0 or above
 * XFG_STEER_QUEUES_MAX, navail 0 or above XFG_STEER_AVAIL_MAX (avail given),
 * an avail entry or skip_queue >= nqueues or naming a queue without a ring, an
 * unknown mode, a flag other than XFG_EGRESS_SWAP_MACS (XFG_EGRESS_MULTIBUF
 * too), umem, rx_descs, verdicts or counts NULL with count != 0 (counts NULL
 * always), a pointer that is not 8-byte aligned, a mask that is not 2^k - 1, a
 * written ring with fewer than count entries, count >= 2^32.  -ENODEV on a
 * host-only context (after these checks; no device pointer is dereferenced
 * before it).
 *
 * Multi-buffer packets (XDP_USE_SG sockets) take xfg_steer_frags_egress below:
 * this call refuses XFG_EGRESS_MULTIBUF, and must not be used on such a batch
 * (it would hash a continuation record as if it began with an Ethernet header
 * and scatter a packet's records over several rings).
 *
 * Not covered: the host-memory path (xfg_classify_xsk_host), the CLI, and the
 * program's round-robin, l4-proto and l4-filter modes.
 */
#define XFG_STEER_QUEUES_MAX 64u
#define XFG_STEER_AVAIL_MAX  256u
#define XFG_STEER_L4_HASH  0u   /* cpumap_l4_hash  */
#define XFG_STEER_L4_SPORT 1u   /* cpumap_l4_sport */
#define XFG_STEER_L4_DPORT 2u   /* cpumap_l4_dport */
#define XFG_QUEUE_NONE 0xffu

struct xfg_steer_queue {        /* one worker's TX ring */
	void *tx_descs;
	uint32_t tx_first, tx_mask;
};

struct xfg_steer {
	size_t sz;                  /* sizeof(struct xfg_steer), for extension */
	void *umem;                 /* device; read for every PASS frame, written with SWAP_MACS */
	const void *rx_descs;
	uint32_t rx_first, rx_mask;
	const struct xfg_steer_queue *queues;  /* HOST, nqueues entries */
	const uint32_t *avail;      /* HOST, navail queue numbers (cpus_available); NULL: identity, navail = nqueues */
	uint32_t nqueues, navail;   /* navail is cpus_count */
	uint32_t mode, skip_queue;
	uint64_t *fill_addrs;       /* NULL: no fill entries written */
	uint32_t fill_first, fill_mask;
	uint64_t count;             /* < 2^32 */
	uint64_t *counts;           /* device, (nqueues + 2) x u64 */
	uint8_t *queue_of;          /* device, count bytes, or NULL */
	uint32_t flags;             /* XFG_EGRESS_SWAP_MACS only (xfg_steer_frags_egress: XFG_EGRESS_MULTIBUF too) */
};

int xfg_steer_egress(xfg_ctx *ctx, int dev, const struct xfg_steer *s,
		     const uint8_t *verdicts, void *stream);

/*
 * Steered egress of multi-buffer packets: every record of a packet follows
 * its head record's queue.  The structure, the queue choice (parse_eth, the
 * three modes, avail, skip_queue), the tables' staging and the stream ordering
 * are xfg_steer_egress's, bit for bit; what differs is what a record is part
 * of.  An XDP program sees only a packet's first buffer, so the head's queue
 * is what cpumap_l4_hash / _sport / _dport return on the head buffer.
 *
 * Packets are formed as xfg_capture_descs_frags forms them.  With v[i] the
 * verdict byte and o[i] the options of record i:
 *   live[i] = v[i] != XFG_VERDICT_NONE
 *   eop[i]  = !(o[i] & XFG_XDP_PKT_CONTD)
 *   head[i] = live[i] && (i == 0 || !live[i-1] || eop[i-1])
 * and a live record belongs to the nearest head at or before it.  So one call
 * serves the output of xfg_classify_descs_frags (count = its counts[1]) and,
 * as a plain array, sk->flat of xfg_classify_socks_frags, whose
 * XFG_VERDICT_NONE bytes keep the sockets apart and mark the trailing
 * incomplete packets.  Both leave every live run ending in an end-of-packet
 * record; this call does not check that: a live run without one is steered by
 * its head like any other.  A packet's record count is not limited.
 *
 * The head decides the whole packet.  A packet whose head byte is
 * XFG_XDP_PASS takes the queue xfg_steer_egress would give the head record's
 * frame (bytes [0, len) at the head's address), and every live record of it
 * goes to that queue's TX ring; a packet whose head byte is anything else
 * hands every live record's chunk to the fill ring.  The other records' verdict
 * bytes count for liveness only, and no UMEM byte of a record that is not a
 * PASS head is read.
 *
 * The k-th live record in record order that takes queue q becomes
 * queues[q].tx_descs[(tx_first + k) & tx_mask]: addr and len as received,
 * options = the RX record's options & XFG_XDP_PKT_CONTD (as xfg_ring_egress
 * with XFG_EGRESS_MULTIBUF), so a packet's records lie adjacent and in order
 * on one ring.  The j-th live record on the fill side writes
 * fill_addrs[(fill_first + j) & fill_mask] = addr & ((1 << 48) - 1)
 * (fill_addrs == NULL: none written).  A record that is not live produces
 * nothing -- no TX record, no fill entry, no count: the caller leaves it on
 * its ring.  counts[q]: the TX records of queue q, per record (as l2fwd's
 * tx_frags counts); counts[nqueues]: the live records on the fill side;
 * counts[nqueues + 1]: the PASS packets whose head parse_eth refused, per
 * packet (their records are among counts[skip_queue]).  queue_of[i]: the
 * packet's queue for every live record of a PASS packet, XFG_QUEUE_NONE for
 * every other record, those that are not live included.
 * XFG_EGRESS_SWAP_MACS touches the head records of PASS packets only.
 *
 * flags: XFG_EGRESS_SWAP_MACS, with or without XFG_EGRESS_MULTIBUF (implied
 * here); every other bit is refused.  If every record is an end of packet and
 * no byte is XFG_VERDICT_NONE, every output byte equals xfg_steer_egress's.
 *
 * -EINVAL: everything xfg_steer_egress refuses, but for XFG_EGRESS_MULTIBUF.
 * -ENODEV on a host-only context, after these checks; no device pointer is
 * touched before it.  count == 0: the counts are zeroed and nothing else is
 * written.  Stream-ordered on @stream, no host synchronisation.
 */
int xfg_steer_frags_egress(xfg_ctx *ctx, int dev, const struct xfg_steer *s,
			   const uint8_t *verdicts, void *stream);

/*
 * A forwarding table (FIB) for xfg_forward_egress below: IPv4 routes with
 * longest-prefix match, and the next hops they name -- what bpf_fib_lookup
 * answers xdp-forward (xdp-forward/xdp_forward.bpf.c:87) from the kernel's
 * route and neighbour tables, as data the caller supplies.
 *
 * A route is (prefix, len, nexthop): prefix in host order (10.0.0.0/8 is
 * 0x0a000000, len 8), no bit set below len; len 0 is the default route;
 * nexthop an index into the next-hop array.  A next hop is what the lookup
 * leaves in fib_params for it: the egress ifindex (never 0), the route's mtu
 * (0: not checked), the two MAC addresses, and ret -- 0 for
 * BPF_FIB_LKUP_RET_SUCCESS, else the non-zero return the lookup gives for this
 * next hop (blackhole, unreachable, prohibit, no neighbour, ...).
 *
 * The table is DIR-24-8 with 16-bit entries: a first table of 2^24 entries
 * (32 MiB) indexed by the address's top 24 bits, 256-entry second-level groups
 * for the /24s that hold a prefix longer than /24, and a dense array of
 * 32-byte next-hop records.  An entry is 0 (no route), next hop + 1, or
 * 0x8000 | group in the first table.  So an address covered by nothing longer
 * than /24 costs one table load, every other two, and "no route" is an entry
 * value.  That format holds XFG_FIB_NEXTHOPS_MAX next hops and
 * XFG_FIB_GROUPS_MAX groups.
 *
 * A FIB is immutable: to change a route, build a new one and pass that to the
 * next call (the old one may be freed once the calls that use it have
 * completed on the device).  The builder keeps a host copy of the tables,
 * which xfg_fib_lookup_host reads; on a host-only context xfg_fib_create
 * builds just that copy (dev is then not looked at), on a device context it
 * also uploads the tables to device @dev once, before it returns.  The arrays
 * passed in are not kept.  IPv6 routes, policy routing (the lookup's tos,
 * l4_protocol, source address and ingress ifindex inputs) and in-place updates
 * are not modelled.
 *
 * xfg_fib_create -- -EINVAL: ctx or out NULL, routes NULL with nroutes != 0,
 * nexthops NULL with nnexthops != 0, dev out of range on a device context, a
 * route with len > 32, with prefix bits set below len or with nexthop >=
 * nnexthops, a next hop with ifindex 0.  -ENOSPC: more than
 * XFG_FIB_NEXTHOPS_MAX next hops, or more than XFG_FIB_GROUPS_MAX /24s with a
 * longer prefix in them.  -EEXIST: the same (prefix, len) given twice.
 * -ENOMEM.  xfg_fib_lookup_host: the longest match's next hop in *nexthop and
 * 0; -ENOENT: no route covers @dst (host order); -EINVAL: fib NULL.
 */
#define XFG_FIB_NEXTHOPS_MAX 32767u
#define XFG_FIB_GROUPS_MAX   32768u

typedef struct xfg_fib xfg_fib;

struct xfg_fib_nexthop {
	uint32_t ifindex;           /* egress port, as fib_params.ifindex comes back; != 0 */
	uint16_t mtu;               /* 0: not checked */
	uint8_t  ret;               /* 0: BPF_FIB_LKUP_RET_SUCCESS; else the lookup's return */
	uint8_t  dmac[6], smac[6];
};

struct xfg_fib_route {
	uint32_t prefix;            /* host order */
	uint32_t nexthop;
	uint8_t  len;
};

int xfg_fib_create(xfg_ctx *ctx, int dev, const struct xfg_fib_route *routes, uint64_t nroutes,
		   const struct xfg_fib_nexthop *nexthops, uint32_t nnexthops, xfg_fib **out);
void xfg_fib_free(xfg_fib *fib);
int xfg_fib_lookup_host(const xfg_fib *fib, uint32_t dst, uint32_t *nexthop);

/*
 * Forwarded egress: where a passed frame goes, decided on the device by a FIB
 * -- "filter, then route".  This is xdp-forward's xdp_fwd_fib_full
 * (xdp-forward/xdp_forward.bpf.c:32-133) with a TX ring in the place of an
 * xdp_tx_ports entry and an xfg_fib in the place of bpf_fib_lookup.
 *
 * Records, verdicts, the fill side, the entry formats, masks, index wrap, ring
 * overlap and stream ordering are xfg_steer_egress's: record i is
 * rx_descs[(rx_first + i) & rx_mask] with verdict byte verdicts[i]; a record
 * whose verdict is not XFG_XDP_PASS hands its chunk to the fill ring.  A PASS
 * record's frame, bytes [0, len) in the UMEM, goes through the program:
 * parse_ethhdr (headers/xdp/parsing_helpers.h:100-134, VLAN_MAX_DEPTH 4), then
 * parse_iphdr (:201-233), the TTL check, the lookup, the xdp_tx_ports check.
 * It gets one reason, the first of these rows that holds:
 *
 *   XFG_FWD_NOT_IP   len < 14, or after up to four 802.1Q/802.1AD tags the
 *                    ethertype is neither IPv4 nor IPv6.  A tag that does not
 *                    fit in the frame ends the loop and leaves the VLAN
 *                    ethertype (:123-124), and so does a fifth tag
 *                    (xdp_forward.bpf.c:45-46,81-83).
 *   XFG_FWD_BAD_HDR  IPv4 and l3 + 20 > len or l3 + 4 * ihl > len, l3 the
 *                    offset behind the tags.  The program has no ihl >= 5
 *                    check, so there is none here (:47-49).
 *   XFG_FWD_TTL      ttl <= 1 (:51-52).
 *   XFG_FWD_V6       the ethertype is IPv6: this FIB has no IPv6 table, and
 *                    every path of the program through a failed lookup returns
 *                    XDP_PASS.  The frame is not parsed further (:62-80,126).
 *   XFG_FWD_NO_ROUTE no prefix covers daddr (:126).
 *   XFG_FWD_NH_RET   the next hop's ret != 0 (:126).
 *   XFG_FWD_FRAG     the next hop's mtu != 0 and ntohs(tot_len) > mtu -- the
 *                    header field, not the record's len (:59,126).
 *   XFG_FWD_NO_PORT  the next hop's ifindex is not among ports (:113-114).
 *   XFG_FWD_OK       forwarded (:104-123).
 *
 * (The program returns XDP_PASS for NO_ROUTE .. NO_PORT alike; their order is
 * this library's own.)  XFG_FWD_OK sends the record to TX ring q, the index of
 * the next hop's ifindex in ports, and rewrites the frame in the UMEM as
 * :116-122 do: ip_decrease_ttl (:23-30) literally -- the check field loaded as
 * the little-endian 16-bit value of its bytes, plus htons(0x0100), plus 1 if
 * that sum is >= 0xFFFF, truncated to 16 bits; ttl - 1 -- then bytes 0..5 =
 * dmac, bytes 6..11 = smac.  The VLAN tags and every other byte of the UMEM
 * keep their values.  Every other PASS frame goes to the stack ring untouched:
 * the ring of the frames the program returns XDP_PASS for.  The descriptors of
 * one batch must name distinct frames.
 *
 * Order within every ring is batch order.  queue_of[i] (when given): q, or
 * nports for the stack ring, or XFG_QUEUE_NONE for a record that is not PASS.
 * reason_of[i] (when given): the reason of a PASS record, XFG_QUEUE_NONE for
 * any other.  counts (device, (nports + 2 + XFG_FWD_REASONS) x u64): counts[q]
 * the TX records of port q, counts[nports] the stack records, counts[nports +
 * 1] the fill-side records (whether their fill entries were written or not),
 * counts[nports + 2 + r] the PASS frames with reason r.  count == 0: the
 * counts are zeroed and nothing else is written.
 *
 * xdp_tx_ports holds 64 entries; this call takes XFG_FWD_PORTS_MAX = 63: the
 * stack ring is the 64th queue of the 64-lane look-back.  ports is HOST memory
 * and may be reused as soon as the call returns: it reaches the device through
 * the pinned staging slots of the socket calls, so the call makes no host
 * synchronisation.  Every port's ring, the stack ring and the fill ring need at
 * least count entries.  The UMEM is read for every PASS frame -- the first 64
 * bytes that lie below len rounded up to 16 (frame starts are 16-byte aligned)
 * -- and written for every forwarded one, within those bytes.
 *
 * Limits: IPv4 only (an IPv6 frame goes to the stack ring with XFG_FWD_V6); 63
 * ports; an immutable FIB.  This call takes single-buffer frames (it would
 * parse a continuation record as a frame); a batch of a socket bound with
 * XDP_USE_SG goes to xfg_forward_frags_egress below.  Many-socket rounds run
 * over the flat array xfg_classify_socks leaves.  Not covered: the host-memory
 * path, the CLI, the xdp_flowtable programs.
 *
 * -EINVAL: everything xfg_steer_egress refuses of the fields the two share,
 * and: fib NULL, of another context or built for another device; nports 0 or
 * above XFG_FWD_PORTS_MAX; ports NULL; a port without a ring, with ifindex 0
 * or with an ifindex given twice; stack.tx_descs NULL; any flag.  -ENODEV on a
 * host-only context, after these checks; no device pointer is dereferenced
 * before it.
 */
#define XFG_FWD_PORTS_MAX 63u
#define XFG_FWD_OK        0u
#define XFG_FWD_NOT_IP    1u
#define XFG_FWD_BAD_HDR   2u
#define XFG_FWD_TTL       3u
#define XFG_FWD_V6        4u
#define XFG_FWD_NO_ROUTE  5u
#define XFG_FWD_NH_RET    6u
#define XFG_FWD_FRAG      7u
#define XFG_FWD_NO_PORT   8u
#define XFG_FWD_REASONS   9u

struct xfg_fwd_port {           /* one egress port: an xdp_tx_ports entry and its TX ring */
	uint32_t ifindex;
	void *tx_descs;
	uint32_t tx_first, tx_mask;
};

struct xfg_forward {
	size_t sz;                  /* sizeof(struct xfg_forward), for extension */
	void *umem;                 /* device; read for every PASS frame, written for every forwarded one */
	const void *rx_descs;
	uint32_t rx_first, rx_mask;
	const xfg_fib *fib;
	const struct xfg_fwd_port *ports;   /* HOST, nports entries: the program's xdp_tx_ports */
	uint32_t nports;
	struct xfg_steer_queue stack;       /* the ring of the frames the program returns XDP_PASS for */
	uint64_t *fill_addrs;       /* NULL: no fill entries written */
	uint32_t fill_first, fill_mask;
	uint64_t count;             /* < 2^32 */
	uint64_t *counts;           /* device, (nports + 2 + XFG_FWD_REASONS) x u64 */
	uint8_t *queue_of, *reason_of;      /* device, count bytes each, or NULL */
	uint32_t flags;             /* xfg_forward_egress: non-zero is refused */
};

int xfg_forward_egress(xfg_ctx *ctx, int dev, const struct xfg_forward *f,
		       const uint8_t *verdicts, void *stream);

/*
 * Forwarded egress of multi-buffer packets: every record of a packet follows
 * its head record's port.  The structure, the program run on a frame, the
 * FIB, the rewrite, the tables' staging and the stream ordering are
 * xfg_forward_egress's, bit for bit; what differs is what a record is part of.
 * An XDP program sees only a packet's first buffer, so the program --
 * xdp_fwd_fib_full -- runs on bytes [0, len) of the head record, and
 * XFG_FWD_FRAG compares the header's tot_len, not any record's len.
 *
 * Packets are formed exactly as xfg_steer_frags_egress forms them (live, eop
 * and head as its comment gives them), so one call serves the output of
 * xfg_classify_descs_frags (count = its counts[1]) and, as a plain array,
 * sk->flat of xfg_classify_socks_frags.  A packet's record count is not
 * limited.
 *
 * The head decides the whole packet:
 *   head byte XFG_XDP_PASS, reason XFG_FWD_OK: every live record of the packet
 *     goes to port q's TX ring, and the head's frame alone is rewritten in the
 *     UMEM (TTL, check field, MACs, as above);
 *   head byte XFG_XDP_PASS, any other reason: every live record goes to the
 *     stack ring, and nothing in the UMEM is written;
 *   any other head byte: every live record's chunk goes to the fill ring.
 * The other records' verdict bytes count for liveness only, and no UMEM byte
 * of a record that is not a PASS head is read or written: a continuation chunk
 * that happens to hold a routable frame is neither followed nor decremented.
 *
 * The k-th live record in record order that takes queue q (a port, or nports:
 * the stack ring) becomes that ring's entry (tx_first + k) & tx_mask: addr and
 * len as received, options = the RX record's options & XFG_XDP_PKT_CONTD, so a
 * packet's records lie adjacent and in order on one ring.  The j-th live
 * record on the fill side writes fill_addrs[(fill_first + j) & fill_mask] =
 * addr & ((1 << 48) - 1) (fill_addrs == NULL: none written).  A record that is
 * not live produces nothing and is counted nowhere.  counts[q] and
 * counts[nports]: TX records, per record; counts[nports + 1]: the live records
 * on the fill side; counts[nports + 2 + r]: the PASS packets with reason r, per
 * packet (only heads are parsed).  queue_of[i] and reason_of[i]: the packet's
 * queue and the packet's reason for every live record of a PASS packet,
 * XFG_QUEUE_NONE for every other record, those that are not live included.
 * The head descriptors of one batch must name distinct frames.
 *
 * Nothing depends on timing: a packet whose records lie in several of the
 * kernel's tiles takes its queue and reason from the tile that parsed its
 * head, never from a second look at a frame that may have been rewritten.
 *
 * flags: XFG_EGRESS_MULTIBUF (implied here) or none; every other bit is
 * refused.  If every record is an end of packet and no byte is
 * XFG_VERDICT_NONE, every output byte -- the rings, queue_of, reason_of, the
 * counts, the UMEM -- equals xfg_forward_egress's.
 *
 * -EINVAL: everything xfg_forward_egress refuses, but for XFG_EGRESS_MULTIBUF.
 * -ENODEV on a host-only context, after these checks; no device pointer is
 * touched before it.  count == 0: the counts are zeroed and nothing else is
 * written.  Stream-ordered on @stream, no host synchronisation; ports reaches
 * the device through the same staging slots.
 */
int xfg_forward_frags_egress(xfg_ctx *ctx, int dev, const struct xfg_forward *f,
			     const uint8_t *verdicts, void *stream);

/*
 * Many sockets over one UMEM: one classify and one egress for a whole poll
 * round.  An AF_XDP application has one socket per NIC queue over a shared
 * UMEM (lib/util/xdpsock.c:1788-1809) and peeks a small batch (batch_size 64,
 * lib/util/xdpsock.c:1682) from each on every round: xsk_l2fwd_all() loops
 * l2fwd() and xsk_rx_drop_all() loops rx_drop() over the num_socks sockets
 * (lib/util/xdpsock.c:1553-1576,1269-1285).  With the per-ring calls above
 * that is one classify and one egress launch a socket, each with a fixed cost
 * far above the work of 64 records; these two calls take all the sockets'
 * batches at once.
 *
 * struct xfg_socks names the sockets: socks is HOST memory, nsocks entries,
 * and may be reused as soon as a call returns (the library keeps its own copy
 * for the device).  Socket s's batch is the count records rx_descs[(rx_first
 * + i) & rx_mask], i < count, as for xfg_classify_descs; count 0 is allowed.
 * With base[s] the sum of count over the sockets before s and total =
 * base[nsocks] (below 2^32), flat packet base[s] + i is socket s's record i.
 * The caller knows every base[s] from its own counts.
 *
 * xfg_classify_socks: the effect of xfg_classify_descs on the plain array of
 * the total records in flat order -- @verdicts is device memory, total bytes,
 * in flat order; verdicts, rule hit counts and per-action statistics are
 * exactly those of nsocks xfg_classify_descs calls, one a socket.  A record is
 * taken as a whole packet (XDP_PKT_CONTD is not looked at).  One kernel
 * gathers the records into a plain descriptor array -- flat (device, total x
 * 16 bytes, 16-byte aligned) when given, else library scratch -- and that
 * array is classified as xfg_classify_descs classifies one of total records:
 * every kernel stays available, xfg_open_opts.descs_min_packets and
 * xfg_last_path behave as for such a call.  A flat array the caller passes is
 * a finished plain descriptor array when the call's work is done:
 * xfg_capture_descs with mask 0xffffffff, xfg_compact over the verdicts and
 * any other per-record call compose with it as they are.
 *
 * xfg_socks_egress: l2fwd() a socket (lib/util/xdpsock.c:1466-1551), all of
 * them in one launch.  The k-th record of socket s, in its own order, whose
 * verdict is XFG_XDP_PASS becomes tx_descs[(tx_first + k) & tx_mask] of that
 * socket: addr and len as received, options 0.  A socket with tx_descs == NULL
 * sends nothing and all its chunks go to the fill side (rx_drop,
 * lib/util/xdpsock.c:1199-1258); its verdicts are not read.  Every other
 * record hands its chunk back, addr & ((1 << 48) - 1):
 *   shared fill ring (e->fill_addrs != NULL, the reference's one umem->fq):
 *     the j-th such record in flat order goes to e->fill_addrs[(e->fill_first
 *     + j) & e->fill_mask]; the sockets' own fill fields are ignored;
 *   per-socket fill rings (e->fill_addrs == NULL; a socket per queue, each
 *     with its own fill ring, xsk_socket__create_shared()): the j-th such
 *     record of socket s goes to that socket's fill_addrs[(fill_first + j) &
 *     fill_mask]; a socket whose fill_addrs is NULL writes none.
 * counts (device, (2 * nsocks + 2) x u64): counts[2s] socket s's TX records,
 * counts[2s + 1] its other records (in either mode, written or not),
 * counts[2 * nsocks] and [2 * nsocks + 1] the two totals.  Ring entries past
 * those counts are not written.  XFG_EGRESS_SWAP_MACS as for xfg_ring_egress
 * (the records that go to a TX ring; e needs sk->umem then).  @verdicts is the
 * flat array xfg_classify_socks wrote.
 *
 * Masks, index wrap and ring overlap are as for xfg_ring_egress.  Each ring
 * that is written needs at least as many entries as can reach it: its socket's
 * count, or total for the shared fill ring.
 *
 * Both calls are stream-ordered on @stream (NULL: the library's stream of the
 * device) and make no host synchronisation: classify then egress on one
 * stream need none between them.  (The socket table reaches the device
 * through a small ring of pinned staging slots; the host waits only if all of
 * them are still in flight.)
 *
 * -EINVAL, both calls: sk == NULL, sz below the structure's size, socks ==
 * NULL, nsocks == 0 or above XFG_SOCKS_MAX, a socket with count != 0 and a
 * NULL or not 8-byte aligned rx_descs, an rx_mask that is not 2^k - 1, count
 * > rx_mask + 1, total >= 2^32.  xfg_classify_socks: umem or verdicts NULL
 * with total != 0, flat not 16-byte aligned.  xfg_socks_egress: e == NULL, sz
 * below the structure's size, counts NULL or not 8-byte aligned, a flag other
 * than XFG_EGRESS_SWAP_MACS (XFG_EGRESS_MULTIBUF too), SWAP_MACS without
 * sk->umem, a ring that is written with a mask that is not 2^k - 1, fewer
 * entries than can reach it or a pointer that is not 8-byte aligned, verdicts
 * NULL where a socket with records has a TX ring.  -ENODEV on a host-only
 * context (after these checks; no device pointer is dereferenced before it).
 * total == 0: xfg_classify_socks launches nothing and changes no statistic,
 * xfg_socks_egress writes zero counts and nothing else.
 *
 * Not covered: sockets over different UMEMs (one call a UMEM), the host-memory
 * path (xfg_classify_xsk_host) and the CLI.  Sockets bound with XDP_USE_SG
 * (multi-buffer packets) take xfg_classify_socks_frags and
 * xfg_socks_frags_egress below; these two calls take a record as a whole
 * packet, and xfg_socks_egress refuses XFG_EGRESS_MULTIBUF.
 */
#define XFG_SOCKS_MAX 1024u

struct xfg_sock {               /* one socket: its peeked RX batch, its TX ring, its fill ring */
	const void *rx_descs;
	uint32_t rx_first, rx_mask;
	void *tx_descs;         /* read by xfg_socks_egress only; NULL: nothing sent */
	uint32_t tx_first, tx_mask;
	uint64_t *fill_addrs;   /* read by xfg_socks_egress in per-socket fill mode only */
	uint32_t fill_first, fill_mask;
	uint32_t count;         /* records peeked from this socket; 0 is allowed */
};

struct xfg_socks {
	size_t sz;                      /* sizeof(struct xfg_socks), for extension */
	const void *umem;               /* device: the UMEM all sockets share */
	const struct xfg_sock *socks;   /* HOST memory, nsocks entries */
	void *flat;                     /* device, total x 16 bytes, or NULL: library scratch */
	uint32_t nsocks;                /* 1 .. XFG_SOCKS_MAX */
};

struct xfg_socks_egress {
	size_t sz;                      /* sizeof(struct xfg_socks_egress), for extension */
	uint64_t *fill_addrs;           /* the shared fill ring, or NULL: every socket's own */
	uint32_t fill_first, fill_mask;
	uint64_t *counts;               /* device, (2 * nsocks + 2) x u64 */
	uint32_t flags;                 /* XFG_EGRESS_SWAP_MACS only */
};

int xfg_classify_socks(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
		       uint8_t *verdicts, void *stream);
int xfg_socks_egress(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
		     const struct xfg_socks_egress *e, const uint8_t *verdicts, void *stream);

/*
 * Multi-buffer packets across many sockets: one classify and one egress for a
 * poll round of sockets bound with XDP_USE_SG.  The bind flag is the
 * application's -- all of its sockets carry it or none does -- so this is what
 * a multi-queue application that receives jumbo frames or GRO aggregates calls
 * in the place of one xfg_classify_descs_frags and one xfg_ring_egress
 * (XFG_EGRESS_MULTIBUF) a socket, each of the former with a host
 * synchronisation of its own.
 *
 * Sockets and flat order are those of struct xfg_socks above: socket s's batch
 * is its count records, base[s] the sum of the counts before it, flat record
 * base[s] + i its record i, total < 2^32.
 *
 * Packets are formed per socket, as l2fwd() forms them on each socket's own
 * ring (lib/util/xdpsock.c:1500-1548).  A packet is a maximal run of
 * consecutive records of one socket's batch ending at the first record whose
 * options & XFG_XDP_PKT_CONTD is 0.  Record 0 of every socket starts a packet,
 * whatever the socket before it ended with; a packet never spans sockets.
 * done[s] is the index + 1 of socket s's last end-of-packet record, 0 if it
 * has none and 0 for an empty socket.  Socket s's records i >= done[s] are its
 * trailing incomplete packet: they are not processed -- no verdict, no rule
 * hit, no statistic -- and the caller leaves them on that ring.
 *
 * xfg_classify_socks_frags: verdicts, rule hit counts and per-action
 * statistics are exactly those of nsocks xfg_classify_descs_frags calls, one a
 * socket, in socket order.  @verdicts is device memory, total bytes, in flat
 * order: every record of a complete packet gets its packet's verdict, and
 * every other record's byte is written as XFG_VERDICT_NONE, so the whole
 * array is defined.  (A deliberate difference from xfg_classify_descs_frags,
 * which leaves those bytes alone: xfg_compact and xfg_capture_descs, whose
 * verdict bytes are below 32, pass over them with nothing added.)  fr->done
 * (HOST, nsocks x u32) receives done[]: what to xsk_ring_cons__release on each
 * socket.  fr->counts (HOST): the complete packets, the records in them (the
 * sum of done[]), the trailing records (total minus that), over all sockets.
 * fr->pkt_of, when given (device, total x u32): the flat packet index of a
 * record in a complete packet -- the number of end-of-packet records before it
 * in flat order -- and XFG_PKT_NONE for the other records.  The packets' head
 * records are classified as xfg_classify_descs classifies a plain array of
 * counts[0] records: xfg_open_opts.descs_min_packets, xfg_last_path and every
 * kernel behave as for such a call.  sk->flat, when given, receives all total
 * records in flat order as in xfg_classify_socks; when NULL no flat array is
 * needed at all.
 *
 * On the device: a pass that finds done[] (and writes flat), the head pass
 * (packet indices, the complete packets' heads gathered into library scratch,
 * the packet count), the read-back of done[] and the packet count, the
 * classify of the heads, and the spread over all total records -- a number of
 * launches that does not depend on nsocks.  The read-back is the call's one
 * host synchronisation, after it has ordered itself behind @stream; the
 * classify and the spread are stream-ordered after it and the call returns
 * without waiting for them.  -EIO if a bounded wait on the device gave up:
 * nothing is classified then and no statistic changes.
 *
 * xfg_socks_frags_egress: l2fwd() a socket with its frags handling
 * (lib/util/xdpsock.c:1521-1542), all sockets in one launch.  sk, e, the fill
 * modes, the layout of counts, masks, index wrap and ring sizes are those of
 * xfg_socks_egress; ring sizes are checked against a socket's count, not its
 * done.  @done is HOST memory, nsocks entries, reusable when the call returns
 * (what xfg_classify_socks_frags wrote); NULL: every record is live.  Socket
 * s's records i >= done[s] are live for nothing: they go to no ring, are
 * counted nowhere, and their verdict bytes are not read.  A live record of a
 * socket with a TX ring whose verdict is XFG_XDP_PASS becomes that socket's
 * next TX record: addr and len as received, options = the RX record's options
 * & XFG_XDP_PKT_CONTD.  Every other live record hands its chunk back: in the
 * shared fill ring at the rank of the live non-PASS records before it in flat
 * order, in its socket's own at the rank within its socket.  counts[2s] =
 * socket s's TX records, counts[2s + 1] = done[s] minus that, and the two
 * totals likewise.  XFG_EGRESS_SWAP_MACS touches head records only: a socket's
 * record 0, and record i iff record i - 1 of the same socket has the bit
 * clear.  flags: XFG_EGRESS_SWAP_MACS, with or without XFG_EGRESS_MULTIBUF
 * (implied here).  No host synchronisation: classify then egress on one stream
 * need none between them beyond the classify's own.
 *
 * -EINVAL: everything xfg_classify_socks and xfg_socks_egress refuse (but for
 * XFG_EGRESS_MULTIBUF); fr == NULL, fr->sz below the structure's size,
 * fr->done == NULL, pkt_of not 4-byte aligned; a flag other than the two;
 * done[s] > count[s].  -ENODEV on a host-only context, after these checks; no
 * device pointer is touched before it.  total == 0: the classify launches
 * nothing, zeroes done[] and counts and changes no statistic; the egress
 * writes zero counts only.
 *
 * Capture by whole packet: xfg_capture_descs_frags over sk->flat with the
 * call's verdicts; the XFG_VERDICT_NONE bytes keep a socket's trailing records
 * and the next socket's head apart (xfg_capture_descs captures record by
 * record, and skips the XFG_VERDICT_NONE records).  A second context on the
 * packets this one passed on: xfg_classify_descs_frags_chain over sk->flat the
 * same way, before xfg_socks_frags_egress.  Not covered: the
 * host-memory ring (xfg_classify_xsk_host), the CLI, sockets over different
 * UMEMs.
 */
#define XFG_VERDICT_NONE 0xffu        /* verdict byte of a record in no complete packet */
#define XFG_PKT_NONE     0xffffffffu  /* pkt_of of such a record */

struct xfg_socks_frags {
	size_t sz;           /* sizeof(struct xfg_socks_frags), for extension */
	uint32_t *done;      /* HOST, out, nsocks x u32: records of socket s in complete packets
	                      * (what to xsk_ring_cons__release on that socket) */
	uint32_t *pkt_of;    /* device, total x u32, 4-byte aligned, or NULL */
	uint64_t counts[3];  /* HOST, out: packets, records in them (sum of done[]), trailing
	                      * records (total - that), over all sockets */
};

int xfg_classify_socks_frags(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
			     struct xfg_socks_frags *fr, uint8_t *verdicts, void *stream);

int xfg_socks_frags_egress(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
			   const struct xfg_socks_egress *e, const uint32_t *done,
			   const uint8_t *verdicts, void *stream);

/*
 * Capture by verdict: the frames of a device-resident batch that a program
 * dropped (or passed, or aborted), as finished pcapng Enhanced Packet Blocks
 * in one contiguous device buffer -- what xdpdump records at a program's exit
 * with the verdict in each record, cut to --snapshot-length
 * (xdp-dump/xdpdump.c:51,100,132,502; lib/util/xpcapng.c:392-479).  Only that
 * buffer crosses PCIe; xfg_pcapng_append() (xdpfilter_io.h) adds it to a file
 * begun with xfg_pcapng_begin() as it is.
 *
 * Frame i is selected if its verdict byte v = verdicts[i] is below 32 and bit
 * v of action_mask is set.  Its block is the one xfg_pcapng_write_captured()
 * writes, byte for byte (the layout is stated there): cap = snaplen ?
 * min(len, snaplen) : len frame bytes, L = 52 + ((cap + 3) & ~3) bytes in
 * all, len the batch's length of the frame (data_end - data: as for the
 * classify calls a fixed-stride slot bounds it), the timestamp ts_ns[i] or
 * ts0, the option epb_verdict = {2 (eBPF XDP), u64 v}.
 *
 * The blocks lie in packet order from out + 0 without gaps: frame k's block
 * starts at the sum of the lengths of the selected frames before it.  A block
 * is written only if it ends at or before out_bytes; starts only grow, so the
 * written blocks are a prefix of the selected frames (a later, smaller frame
 * is not slipped in).  counts[0] = blocks written, counts[1] = their bytes,
 * counts[2] = selected frames not written.  Bytes of out at or past counts[1]
 * are not written.
 *
 * Every source form of the two batch structures is taken, under the alignment
 * and read-past rules stated with them (frame starts 16-byte aligned, readable
 * to the next 16-byte boundary past the end).  A block is shorter than 2^25
 * bytes (64 consecutive ones are addressed with 32 bits).  count < 2^32; byte
 * positions in out are 64-bit.
 *
 * -EINVAL: sz below the structure's size, counts == NULL, out == NULL with
 * out_bytes != 0, out not 16-byte or counts / ts_ns not 8-byte aligned,
 * verdicts == NULL with count != 0, a bad batch (as the classify calls
 * refuse it: a mask that is not 2^k - 1, a stride that is no multiple of 16,
 * ...), count >= 2^32.  -ENODEV on a host-only context.  count == 0 or
 * action_mask == 0 writes three zero counts and nothing else.
 *
 * Stream-ordered on @stream (NULL: the library's stream of the device), as
 * xfg_compact and xfg_ring_egress are: after a classify call on the same
 * stream it needs no host synchronisation.  The call changes no map, counter
 * or statistic.  These two calls take every record as a frame of its own: a
 * multi-buffer packet's records (xfg_classify_descs_frags) are captured whole
 * by xfg_capture_descs_frags below.
 */
struct xfg_capture {
	size_t sz;              /* sizeof(struct xfg_capture), for extension */
	uint32_t action_mask;   /* bit a: capture frames whose verdict byte is a (< 32) */
	uint32_t snaplen;       /* 0: whole frames */
	const uint64_t *ts_ns;  /* device, one per packet; NULL: every frame gets ts0 */
	uint64_t ts0;
	void *out;              /* device, 16-byte aligned */
	uint64_t out_bytes;
	uint64_t *counts;       /* device, 3 x u64 */
};

int xfg_capture(xfg_ctx *ctx, int dev, const struct xfg_batch *batch, const uint8_t *verdicts,
		const struct xfg_capture *cap, void *stream);
int xfg_capture_descs(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
		      const uint8_t *verdicts, const struct xfg_capture *cap, void *stream);

/*
 * Capture by verdict of multi-buffer packets: one block a packet, its
 * records' bytes concatenated.  @batch, @verdicts and @cap are those of
 * xfg_capture_descs (array or wrapping ring, the unaligned-chunk address
 * form, the alignment and read-past rules), and the call serves the output of
 * both multi-buffer classify calls: xfg_classify_descs_frags with count =
 * counts[1], and xfg_classify_socks_frags with sk->flat as a plain array
 * (mask 0xffffffff) of count = total records, whose XFG_VERDICT_NONE bytes
 * mark the records in no complete packet.
 *
 * Packets.  With o[i] record i's options, v[i] its verdict byte and n the
 * count: live[i] = v[i] != XFG_VERDICT_NONE; eop[i] = !(o[i] &
 * XFG_XDP_PKT_CONTD); head[i] = live[i] && (i == 0 || !live[i-1] ||
 * eop[i-1]).  The packet of head h is records h..e, e the smallest index >= h
 * with eop[e]; it exists only if every record h..e is live and e < n.  A run
 * of live records that ends -- at the end of the batch or at a record that is
 * not live -- without an end-of-packet record is no packet: nothing is
 * captured or counted for it.  A packet is selected by its head's verdict
 * byte alone (v[h] < 32 and bit v[h] of action_mask); the bytes of its other
 * records matter only for liveness, and other option bits are ignored.
 *
 * The block of a selected packet is the one xfg_pcapng_write_captured()
 * writes for a frame whose bytes are the records' bytes in order, total =
 * len[h] + ... + len[e] of them: cap = snaplen ? min(total, snaplen) : total,
 * L = 52 + ((cap + 3) & ~3), header dwords 5 and 6 cap and total, the verdict
 * v[h], the timestamp ts_ns[h] (ts_ns stays one entry per record) or ts0, pad
 * bytes zero.  With XFG_CAPTURE_HEAD_ONLY packets are formed the same way but
 * the frame is the head record alone, total = len[h]: what xdpdump sees of a
 * multi-buffer frame (pkt_len = data_end - data, xdp-dump/xdpdump_bpf.c:76-77,
 * xdpdump_xdp.c:51-52).  Placement, overflow and the three counts are as for
 * xfg_capture, over packets.  If every record is an end-of-packet record and
 * no verdict byte is XFG_VERDICT_NONE, output and counts are those of
 * xfg_capture_descs.
 *
 * count < 2^32; a packet's lengths sum below 2^25 - 64; its record count is
 * not limited, and the cost does not grow with it.  Two kernels on the
 * device's stream (a segmented scan over the records, then the copy) and
 * 12 bytes a record of library scratch, grown on demand.  Stream-ordered on
 * @stream with no host synchronisation; no map, counter or statistic changes.
 *
 * -EINVAL: everything xfg_capture_descs refuses, and any flag bit other than
 * XFG_CAPTURE_HEAD_ONLY.  -ENODEV on a host-only context, after the argument
 * checks; no device pointer is touched before it.  count == 0 or action_mask
 * == 0 writes three zero counts and nothing else.
 */
#define XFG_CAPTURE_HEAD_ONLY (1u << 0)

int xfg_capture_descs_frags(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
			    const uint8_t *verdicts, const struct xfg_capture *cap,
			    uint32_t flags, void *stream);

/* Per-action stats summed over devices (the userspace per-CPU sum of
 * lib/util/stats.c:140-172), or for one device. */
int xfg_stats_read(xfg_ctx *ctx, struct xfg_stats_record out[XFG_ACTION_MAX]);
int xfg_stats_read_dev(xfg_ctx *ctx, int dev, struct xfg_stats_record out[XFG_ACTION_MAX]);
int xfg_stats_reset(xfg_ctx *ctx);

/* Wait for all work queued by this library on every device. */
int xfg_sync(xfg_ctx *ctx);

/* ---- device memory helpers (so a C host needs no HIP headers) ---- */
void *xfg_dev_alloc(xfg_ctx *ctx, int dev, size_t bytes);
void xfg_dev_free(xfg_ctx *ctx, int dev, void *p);
int xfg_memcpy_h2d(xfg_ctx *ctx, int dev, void *dst, const void *src, size_t bytes);
int xfg_memcpy_d2h(xfg_ctx *ctx, int dev, void *dst, const void *src, size_t bytes);
void *xfg_host_alloc_pinned(size_t bytes);
void xfg_host_free_pinned(void *p);

/* ---- timing: HIP events on the library's stream for device @dev ---- */
/* Launch classify @iters times back-to-back on the device's stream and
 * return the average kernel duration in ms measured with HIP events recorded
 * on that same stream (used by bench.py for the roofline figure). */
int xfg_classify_timed(xfg_ctx *ctx, int dev, const struct xfg_batch *batch,
		       uint8_t *verdicts, int iters, double *avg_ms);
/* The same for a descriptor batch (xfg_classify_descs): @iters >= 1 launches
 * between the two events, the hit log still pending counted inside the timed
 * region.  -EINVAL for an empty batch. */
int xfg_classify_descs_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
			     uint8_t *verdicts, int iters, double *avg_ms);
/* One xfg_classify_descs_frags call on the library's stream with each of its
 * three steps between two events and waited for: ms[0] the head pass, ms[1]
 * the classify of the heads, ms[2] the spread (0 for a step that did not
 * run). */
int xfg_classify_descs_frags_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
				   struct xfg_frags *fr, uint8_t *verdicts, double ms[3]);
/* One xfg_classify_descs_chain call on the library's stream, timed the same
 * way: ms[0] the select pass, ms[1] the classify of the selected frames, ms[2]
 * the scatter (0 for a step that did not run). */
int xfg_classify_descs_chain_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
				   struct xfg_chain *ch, uint8_t *verdicts, double ms[3]);
/* One xfg_classify_descs_frags_chain call on the library's stream, timed the
 * same way: ms[0] the pre-pass (both kernels), ms[1] the classify of the
 * selected packets' heads, ms[2] the spread (0 for a step that did not run). */
int xfg_classify_descs_frags_chain_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *batch,
					 struct xfg_frags_chain *ch, uint8_t *verdicts, double ms[3]);

/* Streaming-read probe: average duration of a kernel that reads @bytes of
 * device memory at @src with 16-byte non-temporal loads (the achievable HBM
 * read rate next to the spec peak, for the roofline report). */
int xfg_stream_read_timed(xfg_ctx *ctx, int dev, const void *src, uint64_t bytes, int iters,
			  double *avg_ms);

/*
 * Multi-process reduction over RCCL (one process per GPU, one device per
 * context).  Rank 0 calls xfg_comm_unique_id() and distributes the 128-byte
 * id out of band; every rank then calls xfg_comm_init().  xfg_comm_allreduce()
 * sums per-rule hit counters and per-action stats across ranks (ncclUint64,
 * ncclSum, in place on a reduction copy); afterwards xfg_map_lookup() /
 * xfg_stats_read() on every rank return the job-wide totals until the next
 * classify call.  This is the GPU analogue of summing per-CPU values
 * (xdp-filter/xdp-filter.c:93-103).
 */
#define XFG_COMM_ID_BYTES 128
int xfg_comm_unique_id(uint8_t id[XFG_COMM_ID_BYTES]);
int xfg_comm_init(xfg_ctx *ctx, int nranks, int rank, const uint8_t id[XFG_COMM_ID_BYTES]);
int xfg_comm_allreduce(xfg_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* XDPFILTER_GPU_H */

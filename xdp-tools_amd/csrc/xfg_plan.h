/* SPDX-License-Identifier: GPL-2.0 */
/*
 * xfg_plan.h — which classify kernel a batch gets and with what shape, as a
 * pure function of a snapshot (xfg_plan.c): no HIP, no allocation, no lock,
 * no environment, no device pointer.  xfg_ctx.c takes the snapshot, provides
 * the planned scratch and launches; tests/plan_replay.c runs the same
 * function over recorded launches on the CPU.
 */
#ifndef XFG_PLAN_H
#define XFG_PLAN_H

#include <stdint.h>

#include "xfg_layout.h"

/* Default smallest IPv4 map that takes the quotient index (its 2^17 buckets
 * are 4 MiB: below this the canonical table and its prefilter stay in L2). */
#define XFG_QT_MIN_KEYS (1u << 18)
/* AF_XDP descriptor batches below this many packets keep the general kernel
 * (xfg_open_opts.descs_min_packets overrides it): on C3's workload as a
 * descriptor batch the pipelined descriptor mode costs 16.7-17.5 us a launch
 * up to 2^16 packets, the general kernel 13.9-14.3 us up to 2^15 and
 * 16.9-17.5 at 2^16; from 2^17 the pipelined mode is ahead (19.1 against
 * 23.5 us; 1.28x at 2^18, 1.79x at 2^22) -- profiles/r07_c3d_ab.log */
#define XFG_DESCS_PIPE_MIN (1u << 16)
#define XFG_LOG_PEND_MAX 4u   /* quotient-index launches per count kernel */

/* Kernel kinds: the launch's (xfg_plan.kind, xfg_last_path) and the rows of
 * the occupancy and threads tables.  7 and 8 are table rows only: kind 5
 * with its count wave (0: cannot launch), and kind 1's descriptor
 * instantiation (a kind-1 launch whose grid is sized from its own entry). */
enum {
	XFG_KIND_GENERAL = 0, XFG_KIND_PIPE = 1, XFG_KIND_IPV4 = 2, XFG_KIND_SPLIT = 3,
	XFG_KIND_SPLIT_PARSE = 4, XFG_KIND_QT = 5, XFG_KIND_ETH = 6,
	XFG_OCC_CW = 7, XFG_OCC_DESCS = 8, XFG_OCC_KINDS = 9,
};
/* column of the occupancy table: the dynamic LDS a launch takes */
#define XFG_OCC_DCNT 1   /* direct counters */
#define XFG_OCC_NIB  2   /* the port nibble map */
#define XFG_OCC_BLOOM 4  /* the Bloom words (bl_lds) */
#define XFG_OCC_EK   8   /* the Ethernet key table */

/* The measurement knobs of the diagnostics build, one field per XFG_*
 * variable; all zero but the two thresholds = the product (xfg_knobs_init).
 * The product passes no knobs at all (NULL). */
struct xfg_knobs {
	uint32_t window;        /* XFG_WINDOW: 64 / 128 above a 64-byte stride */
	enum { XFG_K_ANY, XFG_K_GENERAL, XFG_K_GENERIC, XFG_K_SPLIT } kernel;   /* XFG_KERNEL */
	uint32_t diag_mask;     /* XFG_DIAG_MASK: pipelined IPv4-key kernel, drop a cost */
	uint64_t tstamp;        /* XFG_TSTAMP: device buffer for the QT kernel's phase stamps */
	int bloom_off;          /* XFG_BLOOM=off: split lookup pass without the prefilter */
	int empty;              /* XFG_EMPTY=1: every table empty, stream + parse only */
	int ek_off;             /* XFG_EK=off: no LDS key table */
	enum { XFG_K_QT_AUTO, XFG_K_QT_OFF, XFG_K_QT_ON } qt;   /* XFG_QT: on = at any size */
	int count_atomic;       /* XFG_COUNT=atomic: no log, no index */
	int log_off;            /* XFG_LOG=off: counters by LDS cache + atomics */
	int cw_off;             /* XFG_CW=off: the count kernel every XFG_LOG_PEND launches */
	uint64_t cw_log_min;    /* XFG_CW_LOG_MIN: packets from which the count wave's log runs */
	int bloom_lds_off;      /* XFG_BLOOM_LDS=off: the Bloom words from memory */
	uint32_t grid_per_cu;   /* XFG_GRID_PER_CU (0: the occupancy table's) */
	int defer_kernel;       /* XFG_DEFER=kernel: xfg_defer_kernel after the QT kernel */
	int v6p_off;            /* XFG_V6P=off: every IPv6 frame deferred */
	uint32_t log_pend;      /* XFG_LOG_PEND: launches per count kernel (0: XFG_LOG_PEND_MAX) */
	uint64_t qt_dyn_min;    /* XFG_QT_DYN_MIN: packets from which the QT waves take tiles as they go */
	uint64_t qt_fold_at;    /* XFG_QT_FOLD_AT: fold after this many packets (0: 2^32 - 1) */
};

void xfg_knobs_init(struct xfg_knobs *k);
/* one variable's value into its field; 0, or -1 for a name that is no knob */
int xfg_knobs_set(struct xfg_knobs *k, const char *name, const char *value);
extern const char *const xfg_knob_names[];   /* NULL-terminated */

struct xfg_plan_in {
	uint32_t feat;                /* the program's XFG_FEAT_* */
	struct {                      /* hash maps: IPv4, IPv6, Ethernet */
		uint32_t count, fmask, bloom_words, nslots;
	} map[3];
	uint32_t flags_differ4;       /* IPv4 slots whose flags differ between devices */
	uint32_t port_count;
	uint32_t ctx_window, qt_min_keys, descs_min;   /* xfg_open_opts */
	int ek_ok;                    /* the Ethernet map can serve as an LDS key table (after ek_refresh) */
	/* the batch */
	uint64_t n;
	uint32_t stride;
	int offsets, aligned16, descs, hwin;
	/* the device, and its images in stream order at the launch */
	int ncu;
	const int (*occ)[2][16];      /* [XFG_OCC_KINDS][window 64, 128][XFG_OCC_* bits] */
	const int (*thr)[2];          /* threads per workgroup [XFG_OCC_KINDS][window] */
	int port_tab_ok;              /* the port image is the small table, not the nibble map */
	uint32_t qt_n, qt_live, qt_nimg, qt_bits, ek_slots;
	const struct xfg_knobs *knobs;   /* NULL: the product */
};

/* What the batch needs brought up to date before its launch can be planned.
 * qt_live is final once ek_ok describes a refreshed table: ask again after
 * the ek_refresh that .ek asked for. */
struct xfg_wants {
	int ek;             /* the Ethernet map as an LDS key table */
	uint32_t qt_live;   /* the quotient index for this live mask (0: none) */
};

struct xfg_plan {
	int kind;
	uint32_t window, pipe, dense, km, v6d, v6p, split, bloom_off;
	int use_ek, use_qt;
	uint32_t dcnt, bl_lds, bl_off[3];
	uint32_t grid, grid_parse, per_wg;
	uint32_t defer_cap, defer_sep, defer_nsrc, defer_grid;
	/* hit log (logs 0: the fields below it are 0, K 1) */
	int logs, cw;
	uint32_t log_span, log_hist, pwide, pcap, K;
	uint32_t qt_dyn;
	int rec_both;       /* split: a second key record */
	struct {            /* scratch the caller provides, bytes (0: none) */
		uint64_t defer, defer_n, tlog, pbuf, pfill, rec, qt_hits;
	} bytes;
};

void xfg_plan_wants(const struct xfg_plan_in *in, struct xfg_wants *w);
void xfg_plan(const struct xfg_plan_in *in, struct xfg_plan *p);

#endif /* XFG_PLAN_H */

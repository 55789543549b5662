/* SPDX-License-Identifier: GPL-2.0 */
/*
 * xfg_ctx.c — host runtime behind include/xdpfilter_gpu.h (plain C over the
 * HIP runtime C API; the kernels live in xfg_kernels.hip).
 *
 * What replaces what in the reference:
 *   program selection     find_prog_file()          xdp-filter/xdp-filter.c:48-60
 *   BPF map CRUD          bpf_map_*_elem() on pinned per-CPU maps
 *                         (xdp-filter/xdp-filter.c:73-157; lib/util/util.h:29-33)
 *   per-CPU value copies  one value per device (flag bytes + hits in HBM)
 *   stats readout         map_get_value_percpu_array  lib/util/stats.c:140-172
 *   prog_lock_acquire     a context mutex           lib/util/util.c:727-767
 */
#define _GNU_SOURCE
#include "xdpfilter_gpu.h"

#include <errno.h>
#include <stddef.h>
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include "xfg_layout.h"
#include "xfg_plan.h"
#include "xfg_table.h"
#include "xfg_fib.h"

/* from xfg_kernels.hip */
int xfg_launch_log_count(const struct xfg_kargs *a, void *stream);
int xfg_launch_classify(uint32_t prog_features, const struct xfg_kargs *a, unsigned grid,
			void *stream);
int xfg_launch_stream_read(const void *src, uint64_t bytes, void *sink, unsigned grid,
			   void *stream);
int xfg_classify_occupancy(uint32_t prog_features, int kind, uint32_t window, size_t dyn);
int xfg_classify_threads(int kind, uint32_t window);
int xfg_launch_compact(const uint8_t *verdicts, uint64_t n, uint32_t action, uint32_t *idx,
		       unsigned long long *count, unsigned long long *status, uint32_t *ticket,
		       unsigned grid, void *stream);
uint64_t xfg_compact_tiles(uint64_t n);
int xfg_launch_egress(const struct xfg_egress_kargs *a, unsigned grid, void *stream);
int xfg_launch_capture(const struct xfg_capture_kargs *a, unsigned grid, void *stream);
int xfg_launch_capture_frags(const struct xfg_capture_frags_kargs *a, unsigned grid, void *stream);
int xfg_launch_frags_heads(const struct xfg_frags_kargs *a, unsigned grid, void *stream);
int xfg_launch_frags_spread(const uint8_t *pv, const uint32_t *pkt_of, uint8_t *verdicts,
			    uint32_t done, unsigned grid, void *stream);
int xfg_launch_chain_select(const struct xfg_chain_kargs *a, unsigned grid, void *stream);
int xfg_launch_chain_scatter(const uint8_t *pv, const uint32_t *idx, uint8_t *verdicts,
			     uint32_t cnt, unsigned grid, void *stream);
int xfg_launch_frags_chain_select(const struct xfg_frags_chain_kargs *a, unsigned grid, void *stream);
int xfg_launch_frags_chain_spread(const uint8_t *pv, const uint32_t *seg, uint8_t *verdicts,
				  uint32_t n, unsigned grid, void *stream);
int xfg_launch_socks_gather(const struct xfg_socks_gather_kargs *a, unsigned grid, void *stream);
int xfg_launch_socks_egress(const struct xfg_socks_kargs *a, unsigned grid, void *stream);
int xfg_launch_socks_frags_heads(const struct xfg_socks_frags_kargs *a, unsigned grid, void *stream);
int xfg_launch_socks_frags_spread(const uint8_t *pv, const uint32_t *pkt_of, uint8_t *verdicts,
				  uint32_t n, unsigned grid, void *stream);
int xfg_launch_steer(const struct xfg_steer_kargs *a, unsigned grid, void *stream);
int xfg_launch_steer_frags(const struct xfg_steer_kargs *a, unsigned grid, void *stream);
int xfg_launch_forward(const struct xfg_fwd_kargs *a, unsigned grid, void *stream);
int xfg_launch_forward_frags(const struct xfg_fwd_kargs *a, unsigned grid, void *stream);
int xfg_launch_socks_frags_egress(const struct xfg_socks_frags_egress_kargs *a, unsigned grid,
				  void *stream);
int xfg_launch_qt_fold(uint32_t *qt_hits, const uint32_t *trans,
		       unsigned long long *hits, uint32_t n, void *stream);

#define NMAPS_HASH 3 /* ipv4, ipv6, ethernet */
#define XFG_HOST_REG_MAX 16 /* registered host buffers per context */
/* host-resident classify: staging slots in flight (each: a chunk's copies,
 * kernel and verdicts on its own stream; the host prepares the next chunk
 * while the others move) */
#ifndef HOST_SLOTS
#define HOST_SLOTS 4
#endif
/* many sockets (xfg_classify_socks, xfg_socks_egress): socket tables on their
 * way to the device at one time; a slot holds the largest table */
#define SOCKS_SLOTS 8
#define SOCKS_SLOT_BYTES ((XFG_SOCKS_FRAGS_TABLE_BYTES(XFG_SOCKS_MAX) + 63) & ~63ull)
_Static_assert(XFG_SOCKS_MAX == XFG_SOCKS_TABLE_MAX, "the kernels' table of bases");

struct dev_map {           /* device arrays of one hash map */
	uint8_t *buckets;      /* (nbuckets + 1) * 64 B: keys, per-device flags, meta */
	uint32_t *bloom;
	unsigned long long *hits;
	unsigned long long *red_hits; /* reduction copy (multi-process) */
};

struct xfg_dev {
	int ordinal;
	int ncu;
	hipStream_t stream;
	hipEvent_t ev0, ev1;
	struct dev_map m[NMAPS_HASH];
	uint8_t *port_flags;
	unsigned long long *port_hits;
	unsigned long long *red_port_hits;
	unsigned long long *stats;      /* 10 */
	unsigned long long *red_stats;  /* 10 */
	void *sink;                     /* stream-read probe sink */
	/* port table (xfg_layout.h): host mirror of this device's port flag
	 * bytes, rebuilt into port_tab before a launch when dirty */
	uint8_t *port_flags_h;
	uint32_t *port_tab;             /* XFG_PORT_TAB entries (ruled ports <= XFG_PORT_TAB_MAX) */
	uint32_t *port_nib;             /* XFG_PORT_NIB_WORDS (more ruled ports) */
	uint32_t port_tab_disp;
	int port_tab_ok, port_tab_dirty;
	/* resident classify workgroups per CU and threads per workgroup:
	 * [kernel kind][window 64, 128][dynamic LDS, XFG_OCC_* bits] (xfg_plan.h) */
	int occ[XFG_OCC_KINDS][2][16];
	int thr[XFG_OCC_KINDS][2];
	/* the Ethernet-key kernel's key table (kind 6), uploaded from ctx->ek
	 * when ek_gen falls behind ctx->ek_gen; params read at launch under
	 * d->lock */
	uint32_t *ek_img;
	uint64_t ek_img_bytes;
	uint32_t ek_gen, ek_slots, ek_disp;
	/* quotient index of the IPv4 map (kind 5 kernel), uploaded from
	 * ctx->qt when qt_gen falls behind ctx->qt_gen; params read at launch
	 * under d->lock */
	uint32_t *qt_img, *qt_trans;
	uint64_t qt_img_bytes, qt_trans_bytes;
	uint32_t qt_gen, qt_bits, qt_seed, qt_live, qt_n, qt_nimg;
	/* the count kernel's QT-order hit counts (xfg_kargs.qt_hits) and
	 * whether a launch may have added to them since the last fold */
	uint32_t *qt_hits;
	uint64_t qt_hits_bytes;
	uint64_t qt_pk;                /* packets classified through the index since the last fold */
	int qt_pending;
	int last_kind;                 /* kernel kind of the last launch (-1: none) */
	/* host-resident classify (xfg_classify_host / xfg_classify_xsk_host),
	 * under host_lock: a gather pool, two fixed-size staging slots of
	 * HOST_CH packets x HOST_WIN bytes (header windows, or whole slots of
	 * a batch with a stride <= HOST_WIN) with their fallback lists, and the
	 * whole-frame fallback staging (FB_BYTES) */
	pthread_mutex_t host_lock;
	struct hpool *pool;
	uint8_t *hs_hbuf[HOST_SLOTS], *hs_dbuf[HOST_SLOTS], *hs_dv[HOST_SLOTS];
	uint32_t *hs_hl[HOST_SLOTS], *hs_dl[HOST_SLOTS];
	uint32_t *hs_fb[HOST_SLOTS], *hs_fbc[HOST_SLOTS], *hs_hfbc[HOST_SLOTS];
	hipStream_t hs_st[HOST_SLOTS];
	hipEvent_t hs_done[HOST_SLOTS];
	uint8_t *fb_h, *fb_d, *fb_dv;   /* fallback frames (pinned / device), verdicts */
	uint64_t *fb_ho, *fb_do;        /* their offsets */
	uint32_t *fb_hl, *fb_dl, *fb_idx;
	pthread_mutex_t lock;           /* launch scratch below + compaction scratch */
	int lock_ok;
	uint32_t *defer;                /* pipelined kernel: deferred-packet lists */
	uint64_t defer_bytes;
	uint32_t *defer_n;              /* ... their fills (xfg_defer_kernel) */
	uint64_t defer_n_bytes;
	uint32_t *tlog, *pfill;         /* hit log: wave regions, slice fills */
	uint16_t *pbuf;                 /* hit log: partition slices */
	uint64_t tlog_bytes, pbuf_bytes, pfill_bytes;
	/* quotient-index logs not yet counted: log_pend launches of log_grid
	 * workgroups, side by side in the partition buffers, counted by one
	 * count kernel with log_args (their shape) -- when the buffers are
	 * full, before any read of the counts (qt_fold_locked) and before a
	 * launch of another shape */
	uint32_t log_pend, log_grid;
	struct xfg_kargs log_args;
	/* (log_cw: the pending log was written in the count wave's mode --
	 * one launch's slices, set log_first of two -- for the next launch's
	 * count wave to take; log_first: the first pending slice) */
	uint32_t log_cw, log_first;
	uint32_t *rec;                  /* split classify: parse-pass records */
	uint64_t rec_bytes;
	unsigned long long *cstatus;    /* verdict compaction, egress, capture: tile status words */
	uint64_t cstatus_cap;
	uint32_t *cticket;
	/* the staged calls' scratch (staged_run()), sized there and used one
	 * call at a time under frags_lock: for multi-buffer batches of one
	 * socket or many (xfg_classify_descs_frags, xfg_classify_socks_frags)
	 * the head records, the per-packet verdicts and, where the caller
	 * passes none, the records' packet indices; for a chained stage the
	 * selected frames' descriptors, their verdicts and their indices */
	pthread_mutex_t frags_lock;
	void *fr_heads;
	uint8_t *fr_pv;
	uint32_t *fr_pkt;
	uint64_t fr_heads_bytes, fr_pv_bytes, fr_pkt_bytes;
	/* a chained stage over a multi-buffer batch
	 * (xfg_classify_descs_frags_chain, under frags_lock): the records'
	 * segments and the segments' ranks, heads and ends (xfg_layout.h); made
	 * by its pre-pass */
	uint32_t *fc_seg;
	uint64_t fc_seg_bytes;
	/* capture of multi-buffer packets (xfg_capture_descs_frags): a record's
	 * bytes of its packet before it, a head's {bytes, records} */
	uint32_t *cf_off;
	unsigned long long *cf_tot;
	uint64_t cf_off_bytes, cf_tot_bytes;
	/* many sockets (xfg_classify_socks, xfg_socks_egress).  The caller's
	 * socket table is host memory it may reuse when a call returns, so each
	 * call copies it (rings and bases, xfg_layout.h) into the next of a ring
	 * of pinned staging slots and from there to the slot's device copy on
	 * the device's stream; the slot's event, recorded behind the kernel that
	 * reads the table, says when both may be written again (under d->lock;
	 * made at first use).  One xfg_classify_socks at a time under
	 * socks_lock, staged_run()'s outer lock for that call: the gathered
	 * records where the caller passes no array, sized by its pre-pass. */
	pthread_mutex_t socks_lock;
	uint8_t *sk_host[SOCKS_SLOTS], *sk_dev[SOCKS_SLOTS];
	hipEvent_t sk_done[SOCKS_SLOTS];
	uint32_t sk_next;
	void *sk_flat;
	uint64_t sk_flat_bytes;
	/* xfg_classify_socks_frags (under frags_lock): pinned room for its one
	 * read-back, the state words from the gave-up word to the end of
	 * done[]; made by its pre-pass at first use */
	unsigned long long *sf_got;
	hipEvent_t ev_user, ev_done;    /* ordering against a caller's stream */
};

struct xfg_ctx {
	pthread_mutex_t lock;
	uint32_t prog_features;
	const char *prog_name;
	int ndev;
	struct xfg_dev *dev;
	struct xfg_table t[NMAPS_HASH];  /* index = map id - 1 */
	/* host-only context: value store for ndev == 0 */
	uint64_t *host_vals[NMAPS_HASH];
	uint64_t *host_port_vals;
	uint8_t *port_flags_host;        /* OR over devices of the port flags */
	uint32_t port_count;
	/* flag-bit census: flag_or[map][slot] = OR over devices of the slot's
	 * flag byte; flag_cnt[map][bit] = slots with that bit (likewise for the
	 * ports).  The kernel skips a lookup whose mask no key carries. */
	uint8_t *flag_or[NMAPS_HASH];
	uint32_t flag_cnt[NMAPS_HASH][8];   /* bit 7: slots whose flags differ between devices */
	/* quotient index of the IPv4 map (xfg_table.h): rebuilt before a
	 * classify that uses it when the map changed (qt_dirty); generation
	 * qt_gen (0 = never built) */
	struct xfg_qt qt;
	int qt_dirty;
	uint32_t qt_gen;
	/* the Ethernet map as the Ethernet-key kernel's LDS key table
	 * (xfg_kargs.ek): rebuilt when an Ethernet flag byte or key changed
	 * (ek_edits moved past ek_built); ek_ok: it can serve (few keys, the
	 * same flags on every device) */
	uint32_t ek_host[XFG_EK_SLOTS_MAX * 4];
	uint32_t ek_slots, ek_disp;
	uint32_t ek_edits, ek_seen;   /* Ethernet map edits; those the table holds */
	uint32_t ek_gen;              /* tables built (0: none yet) */
	int ek_ok;
	uint32_t qt_min_keys;
	uint32_t descs_min;          /* descriptor batches from this size: the pipelined kernel */
	uint32_t window;                /* header window above a 64-byte stride: 64 or 128 */
	uint32_t port_flag_cnt[8];
	/* multi-process reduction */
	ncclComm_t comm;
	int comm_ready;
	int reduced;
	/* host buffers registered for direct DMA (xfg_host_register) */
	pthread_mutex_t reg_lock;
	struct { const uint8_t *p; size_t bytes; } reg[XFG_HOST_REG_MAX];
	int nreg;
};

/* ------------------------------------------------------------------ misc */
static const struct { const char *name; uint32_t feat; } prog_table[] = {
	/* xdp-filter/Makefile:3-6 order; features = each program's _features */
	{ "xdpfilt_dny_udp", XFG_FEAT_UDP | XFG_FEAT_DENY },
	{ "xdpfilt_dny_tcp", XFG_FEAT_TCP | XFG_FEAT_DENY },
	{ "xdpfilt_dny_ip", XFG_FEAT_IPV4 | XFG_FEAT_IPV6 | XFG_FEAT_DENY },
	{ "xdpfilt_dny_eth", XFG_FEAT_ETHERNET | XFG_FEAT_DENY },
	{ "xdpfilt_dny_all", XFG_FEAT_ALL | XFG_FEAT_DENY },
	{ "xdpfilt_alw_udp", XFG_FEAT_UDP | XFG_FEAT_ALLOW },
	{ "xdpfilt_alw_tcp", XFG_FEAT_TCP | XFG_FEAT_ALLOW },
	{ "xdpfilt_alw_ip", XFG_FEAT_IPV4 | XFG_FEAT_IPV6 | XFG_FEAT_ALLOW },
	{ "xdpfilt_alw_eth", XFG_FEAT_ETHERNET | XFG_FEAT_ALLOW },
	{ "xdpfilt_alw_all", XFG_FEAT_ALL | XFG_FEAT_ALLOW },
};

int xfg_select_program(uint32_t features, const char **prog_name, uint32_t *prog_features)
{
	if (!features)
		return -EINVAL;
	for (size_t i = 0; i < sizeof(prog_table) / sizeof(prog_table[0]); i++) {
		if ((prog_table[i].feat & features) == features) {
			if (prog_name)
				*prog_name = prog_table[i].name;
			if (prog_features)
				*prog_features = prog_table[i].feat;
			return 0;
		}
	}
	return -ENOENT;
}

const char *xfg_strerror(int err)
{
	if (err <= -1000)
		return "HIP runtime error";
	return strerror(err < 0 ? -err : err);
}

static int hip_err(hipError_t e)
{
	if (e == hipSuccess)
		return 0;
	if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
		return -ENOMEM;
	if (e == hipErrorNoDevice || e == hipErrorInvalidDevice)
		return -ENODEV;
	return -1000 - (int)e;
}

#define HIPCHK(call)                                  \
	do {                                          \
		int _e = hip_err(call);               \
		if (_e) {                             \
			err = _e;                     \
			goto fail;                    \
		}                                     \
	} while (0)

static int keylen_of(int map)
{
	switch (map) {
	case XFG_MAP_PORTS: return 4;
	case XFG_MAP_IPV4: return 4;
	case XFG_MAP_IPV6: return 16;
	case XFG_MAP_ETHERNET: return 6;
	default: return -EINVAL;
	}
}

/* ------------------------------------------------------------------ gather pool */
/* Persistent worker threads of one device's host path: hpool_run(fn, arg)
 * runs fn(arg, slice, nslices) for every slice, slice 0 on the caller.  As
 * many as the process's CPU set allows, capped by HOST_THREADS; the
 * caller's share of a shared box (whose CPU set shows the whole machine) is
 * XFG_HOST_THREADS, else OMP_NUM_THREADS when it is above 1 -- a value of 1
 * is what torch.distributed.run exports to every rank by default, and taken
 * at its word it would leave each rank's gather one thread.  Performance
 * only: the slices' results do not depend on their count.  xfg_host_threads()
 * reports the size. */
#define HOST_THREADS 16

static int hpool_size(void)
{
	int n = HOST_THREADS;
	cpu_set_t cs;
	if (!sched_getaffinity(0, sizeof(cs), &cs) && CPU_COUNT(&cs) > 0 && CPU_COUNT(&cs) < n)
		n = CPU_COUNT(&cs);
	const char *ht = getenv("XFG_HOST_THREADS");
	const char *omp = getenv("OMP_NUM_THREADS");
	if (ht && atoi(ht) > 0)
		n = atoi(ht) < HOST_THREADS ? atoi(ht) : HOST_THREADS;
	else if (omp && atoi(omp) > 1 && atoi(omp) < n)
		n = atoi(omp);
	return n;
}

int xfg_host_threads(void)
{
	return hpool_size();
}

struct hpool {
	pthread_t th[HOST_THREADS];
	struct hpool_arg {
		struct hpool *p;
		int id;
	} args[HOST_THREADS];
	int nth;                   /* workers (slices 1..nth) */
	pthread_mutex_t mu;
	pthread_cond_t go, done;
	void (*fn)(void *, int, int);
	void *arg;
	unsigned gen;
	int pending, stop;
};

static void *hpool_main(void *v)
{
	struct hpool_arg *w = v;
	struct hpool *p = w->p;
	unsigned seen = 0;
	pthread_mutex_lock(&p->mu);
	for (;;) {
		while (p->gen == seen && !p->stop)
			pthread_cond_wait(&p->go, &p->mu);
		if (p->stop)
			break;
		seen = p->gen;
		void (*fn)(void *, int, int) = p->fn;
		void *arg = p->arg;
		const int n = p->nth + 1;
		pthread_mutex_unlock(&p->mu);
		fn(arg, w->id, n);
		pthread_mutex_lock(&p->mu);
		if (--p->pending == 0)
			pthread_cond_signal(&p->done);
	}
	pthread_mutex_unlock(&p->mu);
	return NULL;
}

static struct hpool *hpool_start(void)
{
	struct hpool *p = calloc(1, sizeof(*p));
	if (!p)
		return NULL;
	pthread_mutex_init(&p->mu, NULL);
	pthread_cond_init(&p->go, NULL);
	pthread_cond_init(&p->done, NULL);
	/* (workers are told their count under the lock, before any run) */
	const int nt = hpool_size();
	pthread_mutex_lock(&p->mu);
	for (int t = 1; t < nt; t++) {
		p->args[t] = (struct hpool_arg){ p, t };
		if (pthread_create(&p->th[t], NULL, hpool_main, &p->args[t]))
			break;
		p->nth = t;
	}
	pthread_mutex_unlock(&p->mu);
	return p;
}

static void hpool_run(struct hpool *p, void (*fn)(void *, int, int), void *arg)
{
	pthread_mutex_lock(&p->mu);
	p->fn = fn;
	p->arg = arg;
	p->pending = p->nth;
	p->gen++;
	pthread_cond_broadcast(&p->go);
	pthread_mutex_unlock(&p->mu);
	fn(arg, 0, p->nth + 1);
	pthread_mutex_lock(&p->mu);
	while (p->pending)
		pthread_cond_wait(&p->done, &p->mu);
	pthread_mutex_unlock(&p->mu);
}

static void hpool_stop(struct hpool *p)
{
	if (!p)
		return;
	pthread_mutex_lock(&p->mu);
	p->stop = 1;
	pthread_cond_broadcast(&p->go);
	pthread_mutex_unlock(&p->mu);
	for (int t = 1; t <= p->nth; t++)
		pthread_join(p->th[t], NULL);
	pthread_cond_destroy(&p->go);
	pthread_cond_destroy(&p->done);
	pthread_mutex_destroy(&p->mu);
	free(p);
}

/* ------------------------------------------------------------------ open */
static void dev_free(struct xfg_dev *d)
{
	hpool_stop(d->pool);
	d->pool = NULL;
	if (d->lock_ok) {
		pthread_mutex_destroy(&d->lock);
		pthread_mutex_destroy(&d->host_lock);
		pthread_mutex_destroy(&d->frags_lock);
		pthread_mutex_destroy(&d->socks_lock);
		d->lock_ok = 0;
	}
	if (hipSetDevice(d->ordinal) != hipSuccess)
		return;
	for (int i = 0; i < NMAPS_HASH; i++) {
		hipFree(d->m[i].buckets);
		hipFree(d->m[i].bloom);
		hipFree(d->m[i].hits);
		hipFree(d->m[i].red_hits);
	}
	hipFree(d->port_flags);
	hipFree(d->port_nib);
	hipFree(d->port_hits);
	hipFree(d->red_port_hits);
	hipFree(d->stats);
	hipFree(d->red_stats);
	hipFree(d->sink);
	hipFree(d->port_tab);
	hipFree(d->qt_img);
	hipFree(d->ek_img);
	hipFree(d->qt_trans);
	hipFree(d->qt_hits);
	free(d->port_flags_h);
	hipFree(d->cstatus);
	for (int k = 0; k < HOST_SLOTS; k++) {
		if (d->hs_st[k])
			hipStreamSynchronize(d->hs_st[k]);
		hipHostFree(d->hs_hbuf[k]);
		hipHostFree(d->hs_hl[k]);
		hipHostFree(d->hs_hfbc[k]);
		hipFree(d->hs_dbuf[k]);
		hipFree(d->hs_dl[k]);
		hipFree(d->hs_dv[k]);
		hipFree(d->hs_fb[k]);
		hipFree(d->hs_fbc[k]);
		if (d->hs_done[k])
			hipEventDestroy(d->hs_done[k]);
		if (d->hs_st[k])
			hipStreamDestroy(d->hs_st[k]);
	}
	hipHostFree(d->fb_h);
	hipHostFree(d->fb_ho);
	hipHostFree(d->fb_hl);
	hipHostFree(d->fb_idx);
	hipFree(d->fb_d);
	hipFree(d->fb_do);
	hipFree(d->fb_dl);
	hipFree(d->fb_dv);
	hipFree(d->defer);
	hipFree(d->defer_n);
	hipFree(d->tlog);
	hipFree(d->pbuf);
	hipFree(d->rec);
	hipFree(d->pfill);
	hipFree(d->cticket);
	hipFree(d->fr_heads);
	hipFree(d->fr_pv);
	hipFree(d->fr_pkt);
	hipFree(d->fc_seg);
	hipFree(d->cf_off);
	hipFree(d->cf_tot);
	for (int k = 0; k < SOCKS_SLOTS; k++) {
		hipHostFree(d->sk_host[k]);
		hipFree(d->sk_dev[k]);
		if (d->sk_done[k])
			hipEventDestroy(d->sk_done[k]);
	}
	hipFree(d->sk_flat);
	hipHostFree(d->sf_got);
	if (d->ev_user)
		hipEventDestroy(d->ev_user);
	if (d->ev_done)
		hipEventDestroy(d->ev_done);
	if (d->ev0)
		hipEventDestroy(d->ev0);
	if (d->ev1)
		hipEventDestroy(d->ev1);
	if (d->stream)
		hipStreamDestroy(d->stream);
}

static int dev_init(xfg_ctx *ctx, struct xfg_dev *d)
{
	int err = 0;
	hipDeviceProp_t prop;

	pthread_mutex_init(&d->lock, NULL);
	pthread_mutex_init(&d->host_lock, NULL);
	pthread_mutex_init(&d->frags_lock, NULL);
	pthread_mutex_init(&d->socks_lock, NULL);
	d->lock_ok = 1;
	HIPCHK(hipSetDevice(d->ordinal));
	HIPCHK(hipGetDeviceProperties(&prop, d->ordinal));
	d->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	HIPCHK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
	HIPCHK(hipEventCreate(&d->ev0));
	HIPCHK(hipEventCreate(&d->ev1));
	for (int i = 0; i < NMAPS_HASH; i++) {
		const struct xfg_table *t = &ctx->t[i];
		size_t ns = (size_t)t->nslots + 1;
		HIPCHK(hipMalloc((void **)&d->m[i].buckets, xfg_table_img_bytes(t)));
		HIPCHK(hipMalloc((void **)&d->m[i].bloom, (size_t)t->bloom_words * 4));
		HIPCHK(hipMalloc((void **)&d->m[i].hits, ns * 8));
		HIPCHK(hipMemset(d->m[i].buckets, 0, xfg_table_img_bytes(t)));
		HIPCHK(hipMemset(d->m[i].bloom, 0, (size_t)t->bloom_words * 4));
		HIPCHK(hipMemset(d->m[i].hits, 0, ns * 8));
	}
	HIPCHK(hipMalloc((void **)&d->port_flags, XFG_PORT_MAP_ENTRIES));
	HIPCHK(hipMalloc((void **)&d->port_nib, XFG_PORT_NIB_WORDS * 4));
	HIPCHK(hipMalloc((void **)&d->port_hits, XFG_PORT_MAP_ENTRIES * 8));
	HIPCHK(hipMemset(d->port_flags, 0, XFG_PORT_MAP_ENTRIES));
	HIPCHK(hipMemset(d->port_hits, 0, XFG_PORT_MAP_ENTRIES * 8));
	HIPCHK(hipMalloc((void **)&d->stats, 10 * 8));
	HIPCHK(hipMemset(d->stats, 0, 10 * 8));
	HIPCHK(hipMalloc(&d->sink, 16 * 65536));
	HIPCHK(hipMalloc((void **)&d->port_tab, XFG_PORT_TAB * 4));
	d->port_flags_h = calloc(XFG_PORT_MAP_ENTRIES, 1);
	if (!d->port_flags_h) {
		err = -ENOMEM;
		goto fail;
	}
	d->port_tab_dirty = 1;
	d->last_kind = -1;
	HIPCHK(hipEventCreateWithFlags(&d->ev_user, hipEventDisableTiming));
	HIPCHK(hipEventCreateWithFlags(&d->ev_done, hipEventDisableTiming));

	for (int k = 0; k < XFG_OCC_KINDS; k++)
		for (int w = 0; w < 2; w++) {
			d->thr[k][w] = xfg_classify_threads(k, w ? 128 : 64);
			for (int c = 0; c < 16; c++)
				d->occ[k][w][c] = xfg_classify_occupancy(
					ctx->prog_features, k, w ? 128 : 64,
					(c & XFG_OCC_DCNT ? XFG_DCNT_MAX * 4 : 0) + (c & XFG_OCC_NIB ? XFG_PORT_NIB_WORDS * 4 : 0) +
					(c & XFG_OCC_BLOOM ? XFG_BLOOM_LDS_MAX * 4 : 0) +
					(c & XFG_OCC_EK ? 12 + XFG_EK_SLOTS_MAX * 16 : 0) +
					(k == XFG_OCC_CW ? 16 + XFG_CW_HIST_MAX * 4 : 0));
		}
	/* (a query past the LDS a workgroup can have may leave an error behind:
	 * not a launch's) */
	(void)hipGetLastError();
	HIPCHK(hipDeviceSynchronize());
	return 0;
fail:
	return err;
}

int xfg_open(xfg_ctx **out, const struct xfg_open_opts *opts)
{
	int err;
	xfg_ctx *ctx;

	if (!out || !opts)
		return -EINVAL;
	*out = NULL;
	ctx = calloc(1, sizeof(*ctx));
	if (!ctx)
		return -ENOMEM;
	pthread_mutex_init(&ctx->lock, NULL);
	pthread_mutex_init(&ctx->reg_lock, NULL);
	err = xfg_select_program(opts->features, &ctx->prog_name, &ctx->prog_features);
	if (err)
		goto fail;

	uint32_t seed = opts->hash_seed ? opts->hash_seed : 0x5eed1234u;
	ctx->qt_min_keys = XFG_QT_MIN_KEYS;
	if (opts->sz >= offsetof(struct xfg_open_opts, qt_min_keys) + sizeof(uint32_t) && opts->qt_min_keys)
		ctx->qt_min_keys = opts->qt_min_keys;
	ctx->descs_min = XFG_DESCS_PIPE_MIN;
	if (opts->sz >= offsetof(struct xfg_open_opts, descs_min_packets) + sizeof(uint32_t) &&
	    opts->descs_min_packets)
		ctx->descs_min = opts->descs_min_packets;
	ctx->window = 64;
	if (opts->sz >= offsetof(struct xfg_open_opts, window) + sizeof(uint32_t) && opts->window) {
		if (opts->window != 64 && opts->window != 128) {
			err = -EINVAL;
			goto fail;
		}
		ctx->window = opts->window;
	}
	uint32_t cap4 = opts->ipv4_capacity ? opts->ipv4_capacity : XFG_DEFAULT_MAP_CAPACITY;
	uint32_t cap6 = opts->ipv6_capacity ? opts->ipv6_capacity : XFG_DEFAULT_MAP_CAPACITY;
	uint32_t cape = opts->eth_capacity ? opts->eth_capacity : XFG_DEFAULT_MAP_CAPACITY;
	if ((err = xfg_table_init(&ctx->t[0], 4, cap4, seed)) ||
	    (err = xfg_table_init(&ctx->t[1], 16, cap6, seed ^ 0x6a09e667u)) ||
	    (err = xfg_table_init(&ctx->t[2], 6, cape, seed ^ 0xbb67ae85u)))
		goto fail;
	for (int i = 0; i < NMAPS_HASH; i++) {
		ctx->flag_or[i] = calloc((size_t)ctx->t[i].nslots + 1, 1);
		if (!ctx->flag_or[i]) {
			err = -ENOMEM;
			goto fail;
		}
	}
	ctx->port_flags_host = calloc(XFG_PORT_MAP_ENTRIES, 1);
	if (!ctx->port_flags_host) {
		err = -ENOMEM;
		goto fail;
	}

	ctx->ndev = opts->ndev > 0 ? opts->ndev : 0;
	if (!ctx->ndev) {
		for (int i = 0; i < NMAPS_HASH; i++) {
			ctx->host_vals[i] = calloc((size_t)ctx->t[i].nslots + 1, 8);
			if (!ctx->host_vals[i]) {
				err = -ENOMEM;
				goto fail;
			}
		}
		ctx->host_port_vals = calloc(XFG_PORT_MAP_ENTRIES, 8);
		if (!ctx->host_port_vals) {
			err = -ENOMEM;
			goto fail;
		}
	} else {
		int count = 0;
		if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
			err = -ENODEV;
			goto fail;
		}
		ctx->dev = calloc(ctx->ndev, sizeof(*ctx->dev));
		if (!ctx->dev) {
			err = -ENOMEM;
			goto fail;
		}
		for (int i = 0; i < ctx->ndev; i++) {
			ctx->dev[i].ordinal = opts->devices ? opts->devices[i] : i;
			if (ctx->dev[i].ordinal < 0 || ctx->dev[i].ordinal >= count) {
				err = -ENODEV;
				goto fail;
			}
			if ((err = dev_init(ctx, &ctx->dev[i])))
				goto fail;
		}
	}
	*out = ctx;
	return 0;
fail:
	xfg_close(ctx);
	return err;
}

void xfg_close(xfg_ctx *ctx)
{
	if (!ctx)
		return;
	if (ctx->comm_ready)
		ncclCommDestroy(ctx->comm);
	for (int i = 0; i < ctx->ndev && ctx->dev; i++)
		dev_free(&ctx->dev[i]);
	for (int i = 0; i < ctx->nreg; i++)
		hipHostUnregister((void *)ctx->reg[i].p);
	pthread_mutex_destroy(&ctx->reg_lock);
	free(ctx->dev);
	for (int i = 0; i < NMAPS_HASH; i++) {
		xfg_table_free(&ctx->t[i]);
		free(ctx->host_vals[i]);
		free(ctx->flag_or[i]);
	}
	xfg_qt_free(&ctx->qt);
	free(ctx->host_port_vals);
	free(ctx->port_flags_host);
	pthread_mutex_destroy(&ctx->lock);
	free(ctx);
}

const char *xfg_prog_name(const xfg_ctx *ctx) { return ctx ? ctx->prog_name : NULL; }

int xfg_last_path(const xfg_ctx *ctx, int dev)
{
	if (!ctx || dev < 0 || dev >= ctx->ndev)
		return -EINVAL;
	return ctx->dev[dev].last_kind < 0 ? -ENOENT : ctx->dev[dev].last_kind;
}
uint32_t xfg_prog_features(const xfg_ctx *ctx) { return ctx ? ctx->prog_features : 0; }
int xfg_num_devices(const xfg_ctx *ctx) { return ctx ? ctx->ndev : -EINVAL; }

/* ------------------------------------------------------------------ maps */
static int dev_read(struct xfg_dev *d, void *dst, const void *src, size_t n)
{
	int err = hip_err(hipSetDevice(d->ordinal));
	if (!err)
		err = hip_err(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, d->stream));
	if (!err)
		err = hip_err(hipStreamSynchronize(d->stream));
	return err;
}

static int dev_write(struct xfg_dev *d, void *dst, const void *src, size_t n)
{
	int err = hip_err(hipSetDevice(d->ordinal));
	if (!err)
		err = hip_err(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, d->stream));
	if (!err)
		err = hip_err(hipStreamSynchronize(d->stream));
	return err;
}

static unsigned long long *hits_view(xfg_ctx *ctx, struct xfg_dev *d, int mi)
{
	return ctx->reduced ? d->m[mi].red_hits : d->m[mi].hits;
}

/* Count the pending quotient-index logs into the QT-order counts (d->lock
 * held): one count kernel over every pending launch's slices. */
static int log_flush_locked(struct xfg_dev *d)
{
	if (!d->log_pend)
		return 0;
	struct xfg_kargs c = d->log_args;
	c.pcount = d->log_pend * d->log_grid;
	c.pfirst = d->log_first;   /* (the count wave's mode: the set of the last launch) */
	c.cw_n = 0;
	d->log_pend = 0;
	int err = hip_err(hipSetDevice(d->ordinal));
	if (!err)
		err = xfg_launch_log_count(&c, d->stream);
	return err;
}

/* Both halves of the QT-order counts (the log's and the atomics',
 * xfg_kargs.qt_hitx) into the canonical counters, one fold each. */
static int qt_fold_launch(struct xfg_dev *d)
{
	int err = xfg_launch_qt_fold(d->qt_hits, d->qt_trans, d->m[0].hits, d->qt_n, d->stream);
	if (!err)
		err = xfg_launch_qt_fold(d->qt_hits + d->qt_n, d->qt_trans, d->m[0].hits, d->qt_n, d->stream);
	return err;
}

/* Add @d's QT-order hit counts into its canonical IPv4 counters, through the
 * index's current qt_trans (d->lock held): in stream order after every
 * classify that counted into them (and after the count kernel of every
 * log still pending). */
static int qt_fold_locked(struct xfg_dev *d)
{
	int err = log_flush_locked(d);
	if (err || !d->qt_pending)
		return err;
	err = hip_err(hipSetDevice(d->ordinal));
	if (!err)
		err = qt_fold_launch(d);
	if (!err)
		err = hip_err(hipStreamSynchronize(d->stream));
	if (!err) {
		d->qt_pending = 0;
		d->qt_pk = 0;
	}
	return err;
}

/* The same fold queued on the device stream with no wait (d->lock held):
 * before a launch whose packets could take a 32-bit QT-order count past
 * 2^32 - 1 (xfg_kargs.qt_hits). */
static int qt_fold_queued(struct xfg_dev *d)
{
	int err = log_flush_locked(d);
	if (!err)
		err = qt_fold_launch(d);
	if (!err)
		d->qt_pk = 0;
	return err;
}

/* Before the IPv4 map's counters are read, written or reduced (ctx->lock
 * held): fold every device's QT-order counts. */
static int qt_fold(xfg_ctx *ctx, int mi)
{
	int err = 0;
	for (int i = 0; mi == 0 && i < ctx->ndev && !err; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		pthread_mutex_lock(&d->lock);
		err = qt_fold_locked(d);
		pthread_mutex_unlock(&d->lock);
	}
	return err;
}

/* Read the per-device values of @slot of hash map @mi (0..2). */
static int slot_values(xfg_ctx *ctx, int mi, uint64_t slot, uint64_t *vals)
{
	if (!ctx->ndev) {
		vals[0] = ctx->host_vals[mi][slot];
		return 0;
	}
	const struct xfg_table *t = &ctx->t[mi];
	int e0 = qt_fold(ctx, mi);
	if (e0)
		return e0;
	for (int i = 0; i < ctx->ndev; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		uint8_t f;
		unsigned long long h;
		int err = dev_read(d, &f, d->m[mi].buckets + xfg_table_flag_off(t, slot), 1);
		if (!err)
			err = dev_read(d, &h, hits_view(ctx, d, mi) + slot, 8);
		if (err)
			return err;
		vals[i] = (h << XFG_COUNTER_SHIFT) | f;
	}
	return 0;
}

static void census(uint32_t *cnt, uint8_t old, uint8_t f)
{
	for (int b = 0; b < 8; b++) {
		cnt[b] -= (old >> b) & 1;
		cnt[b] += (f >> b) & 1;
	}
}

static uint32_t census_mask(const uint32_t *cnt)
{
	uint32_t m = 0;
	for (int b = 0; b < 6; b++)
		if (cnt[b])
			m |= 1u << b;
	return m;
}

/* @any / @all: the OR / AND over devices of the slot's flag byte (bit 7 of
 * the census byte records that they differ).  A changed IPv4 flag byte
 * marks the quotient index for a rebuild unless @patch (a single edit, which
 * slot_store applies to the index in place); returns the old byte. */
static uint8_t flags_note(xfg_ctx *ctx, int mi, uint64_t slot, uint8_t any, uint8_t all, int patch)
{
	const uint8_t f = any | (any != all ? 0x80 : 0), old = ctx->flag_or[mi][slot];
	census(ctx->flag_cnt[mi], old, f);
	if (mi == 2)   /* (every key insert and delete passes here) */
		ctx->ek_edits++;
	ctx->flag_or[mi][slot] = f;
	if (mi == 0 && old != f && !patch)
		ctx->qt_dirty = 1;
	return old;
}

/* One IPv4 key's flag byte went from @old to @nw (ctx->lock held, every
 * device's QT-order counts folded): enter it into or take it out of the
 * quotient index in place (xfg_qt_patch) and send the one bucket and its
 * trans[] entries to every device whose copy was current; a change of the
 * index's size (bits follow the key count) leaves a full rebuild to the
 * next classify, as before.  @key: the key bytes (NULL: read from the
 * table, where the key still is). */
static int qt_edit(xfg_ctx *ctx, uint64_t slot, const void *key, uint8_t old, uint8_t nw)
{
	struct xfg_qt *q = &ctx->qt;
	if (ctx->qt_dirty || !ctx->qt_gen || !q->img)
		return 0;   /* (rebuilt before its next use anyway) */
#ifdef XFG_DIAG
	const char *po = getenv("XFG_QT_PATCH");   /* "off": every edit rebuilds (round 3) */
	if (po && !strcmp(po, "off")) {
		ctx->qt_dirty = 1;
		return 0;
	}
#endif
	/* per image: does the key enter or leave it */
	int chg[2] = { 0, 0 }, any = 0;
	for (uint32_t im = 0; im < q->nimg; im++) {
		const uint32_t mk = xfg_qt_img_mask(q->live, q->nimg, im);
		const int was = (old & mk) == mk, is = (nw & mk) == mk;
		chg[im] = was == is ? 0 : (is ? 1 : -1);
		any |= chg[im];
	}
	/* one image for both directions holds only keys with both or neither:
	 * a key with exactly one direction needs the second image (rebuild) */
	if (q->live == 3 && q->nimg == 1 && ((nw & 3) == 1 || (nw & 3) == 2)) {
		ctx->qt_dirty = 1;
		return 0;
	}
	if (!any)
		return 0;
	if (xfg_qt_bits_for(ctx->t[0].count) != q->bits) {
		ctx->qt_dirty = 1;
		return 0;
	}
	uint32_t k;
	if (key)
		memcpy(&k, key, 4);
	else if (xfg_table_slot_key(&ctx->t[0], slot, &k)) {
		ctx->qt_dirty = 1;
		return 0;
	}
	uint32_t bk[2] = { 0, 0 };
	for (uint32_t im = 0; im < q->nimg; im++)
		if (chg[im])
			bk[im] = xfg_qt_patch(q, im, k, (uint32_t)slot, chg[im] > 0);
	uint32_t gen = ctx->qt_gen + 1;
	if (!gen)
		gen = 1;
	int err = 0;
	for (int i = 0; i < ctx->ndev; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		pthread_mutex_lock(&d->lock);
		/* (a classify launched since slot_store's fold counted through the
		 * old bucket: fold it in the same lock section as the bucket write,
		 * as qt_refresh does, so no count is read through the new trans[]) */
		int e = qt_fold_locked(d);
		if (e) {
			if (!err)
				err = e;
		} else if (d->qt_gen == ctx->qt_gen) {
			for (uint32_t im = 0; im < q->nimg && !e; im++) {
				if (!chg[im])
					continue;
				const uint64_t o = (uint64_t)im * q->nslots + (uint64_t)bk[im] * XFG_QT_SLOTS;
				e = dev_write(d, (uint8_t *)d->qt_img + o * 2, q->img + o, XFG_QT_BUCKET);
				if (!e)
					e = dev_write(d, d->qt_trans + o, q->trans + o, XFG_QT_SLOTS * 4);
			}
			if (!e)
				d->qt_gen = gen;
			else if (!err)
				err = e;
		}
		pthread_mutex_unlock(&d->lock);
	}
	ctx->qt_gen = gen;
	if (err)   /* (a device whose copy may not match the map: rebuild before the next use) */
		ctx->qt_dirty = 1;
	return err;
}

static int slot_store(xfg_ctx *ctx, int mi, uint64_t slot, const uint64_t *vals, const void *key)
{
	uint8_t any = 0, all = 63;
	for (int i = 0; i < (ctx->ndev ? ctx->ndev : 1); i++) {
		any |= vals[i] & 63;
		all &= vals[i] & 63;
	}
	const uint8_t old = flags_note(ctx, mi, slot, any, all, ctx->ndev != 0);
	if (!ctx->ndev) {
		ctx->host_vals[mi][slot] = vals[0];
		return 0;
	}
	const struct xfg_table *t = &ctx->t[mi];
	int e0 = qt_fold(ctx, mi);
	if (!e0 && mi == 0 && old != ctx->flag_or[0][slot])
		e0 = qt_edit(ctx, slot, key, old, ctx->flag_or[0][slot]);
	if (e0) {
		if (mi == 0)   /* (flags_note skipped the rebuild mark for the patch that failed) */
			ctx->qt_dirty = 1;
		return e0;
	}
	for (int i = 0; i < ctx->ndev; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		uint8_t f = vals[i] & 63;
		unsigned long long h = vals[i] >> XFG_COUNTER_SHIFT;
		int err = dev_write(d, d->m[mi].buckets + xfg_table_flag_off(t, slot), &f, 1);
		if (!err)
			err = dev_write(d, d->m[mi].hits + slot, &h, 8);
		if (err)
			return err;
	}
	return 0;
}

/* Push the key bytes of @slot (host image) to every device. */
static int push_key(xfg_ctx *ctx, int mi, uint64_t slot)
{
	const struct xfg_table *t = &ctx->t[mi];
	uint64_t off = xfg_table_key_off(t, slot);
	for (int i = 0; i < ctx->ndev; i++) {
		int err = dev_write(&ctx->dev[i], ctx->dev[i].m[mi].buckets + off, t->img + off,
				    t->slot_bytes);
		if (err)
			return err;
	}
	return 0;
}

static int push_bloom(xfg_ctx *ctx, int mi, int64_t word)
{
	const struct xfg_table *t = &ctx->t[mi];
	for (int i = 0; i < ctx->ndev; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		int err = word < 0 ? dev_write(d, d->m[mi].bloom, t->bloom, (size_t)t->bloom_words * 4)
				   : dev_write(d, d->m[mi].bloom + word, t->bloom + word, 4);
		if (err)
			return err;
	}
	return 0;
}

struct meta_push { xfg_ctx *ctx; int mi; int err; };

static void meta_changed(void *arg, uint32_t b)
{
	struct meta_push *mp = arg;
	xfg_ctx *ctx = mp->ctx;
	uint64_t off = (uint64_t)b * XFG_BUCKET_BYTES + XFG_META_OFF;
	for (int i = 0; i < ctx->ndev && !mp->err; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		mp->err = dev_write(d, d->m[mp->mi].buckets + off, ctx->t[mp->mi].img + off, 4);
	}
}

static int port_key(const void *key, uint32_t *k)
{
	memcpy(k, key, 4);
	return *k < XFG_PORT_MAP_ENTRIES ? 0 : -ENOENT;
}

/* Track which ports have any flag on any device: port_count (the empty-map
 * skip) and the flag census. */
static int port_flags_note(xfg_ctx *ctx, uint32_t k, uint8_t f)
{
	census(ctx->port_flag_cnt, ctx->port_flags_host[k], f);
	if (!ctx->port_flags_host[k] && f)
		ctx->port_count++;
	else if (ctx->port_flags_host[k] && !f)
		ctx->port_count--;
	ctx->port_flags_host[k] = f;
	return 0;
}

int xfg_map_lookup(xfg_ctx *ctx, int map, const void *key, uint64_t *vals)
{
	int err = 0;
	if (!ctx || !key || !vals || keylen_of(map) < 0)
		return -EINVAL;
	pthread_mutex_lock(&ctx->lock);
	if (map == XFG_MAP_PORTS) {
		uint32_t k;
		if ((err = port_key(key, &k)))
			goto out;
		if (!ctx->ndev) {
			vals[0] = ctx->host_port_vals[k];
			goto out;
		}
		for (int i = 0; i < ctx->ndev && !err; i++) {
			struct xfg_dev *d = &ctx->dev[i];
			uint8_t f;
			unsigned long long h = 0;
			err = dev_read(d, &f, d->port_flags + k, 1);
			if (!err)
				err = dev_read(d, &h, (ctx->reduced ? d->red_port_hits : d->port_hits) + k, 8);
			vals[i] = (h << XFG_COUNTER_SHIFT) | f;
		}
		goto out;
	}
	int mi = map - 1;
	int64_t s = xfg_table_find(&ctx->t[mi], key);
	if (s < 0) {
		err = -ENOENT;
		goto out;
	}
	err = slot_values(ctx, mi, (uint64_t)s, vals);
out:
	pthread_mutex_unlock(&ctx->lock);
	return err;
}

static int port_store(xfg_ctx *ctx, uint32_t k, const uint64_t *vals)
{
	int err = 0;
	uint8_t any = 0;
	if (!ctx->ndev) {
		ctx->host_port_vals[k] = vals[0];
		any = vals[0] & 63;
	}
	for (int i = 0; i < ctx->ndev && !err; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		uint8_t f = vals[i] & 63;
		unsigned long long h = vals[i] >> XFG_COUNTER_SHIFT;
		any |= f;
		d->port_flags_h[k] = f;
		d->port_tab_dirty = 1;
		err = dev_write(d, d->port_flags + k, &f, 1);
		if (!err)
			err = dev_write(d, d->port_hits + k, &h, 8);
	}
	if (!err)
		err = port_flags_note(ctx, k, any);
	return err;
}

int xfg_map_update(xfg_ctx *ctx, int map, const void *key, const uint64_t *vals)
{
	int err = 0;
	if (!ctx || !key || !vals || keylen_of(map) < 0)
		return -EINVAL;
	pthread_mutex_lock(&ctx->lock);
	ctx->reduced = 0;
	if (map == XFG_MAP_PORTS) {
		uint32_t k;
		if (port_key(key, &k))
			err = -E2BIG; /* array map: index out of range */
		else
			err = port_store(ctx, k, vals);
		goto out;
	}
	int mi = map - 1;
	struct xfg_table *t = &ctx->t[mi];
	int64_t s = xfg_table_find(t, key);
	if (s < 0) {
		struct meta_push mp = { ctx, mi, 0 };
		int64_t bw = -1;
		s = xfg_table_insert(t, key, ctx->ndev ? meta_changed : NULL, &mp, &bw);
		if (s < 0) {
			err = (int)s;
			goto out;
		}
		if ((err = mp.err))
			goto out;
		if (ctx->ndev && (uint64_t)s != t->nslots) {
			err = push_key(ctx, mi, (uint64_t)s);
			if (!err && bw >= 0)
				err = push_bloom(ctx, mi, bw);
		}
		if (err)
			goto out;
	}
	err = slot_store(ctx, mi, (uint64_t)s, vals, key);
out:
	pthread_mutex_unlock(&ctx->lock);
	return err;
}

int xfg_map_delete(xfg_ctx *ctx, int map, const void *key)
{
	int err = 0;
	if (!ctx || !key || keylen_of(map) < 0)
		return -EINVAL;
	if (map == XFG_MAP_PORTS)
		return -EINVAL; /* BPF array maps do not support delete */
	pthread_mutex_lock(&ctx->lock);
	int mi = map - 1;
	struct xfg_table *t = &ctx->t[mi];
	int64_t s = xfg_table_remove(t, key);
	if (s < 0) {
		err = (int)s;
		goto out;
	}
	{
		uint64_t zero[64] = { 0 };
		uint64_t *z = ctx->ndev > 64 ? calloc(ctx->ndev, 8) : zero;
		if (!z) {
			err = -ENOMEM;
			goto out;
		}
		err = slot_store(ctx, mi, (uint64_t)s, z, key);
		if (z != zero)
			free(z);
	}
	if (!err && (uint64_t)s != t->nslots && ctx->ndev)
		err = push_key(ctx, mi, (uint64_t)s);
	if (!err && xfg_table_bloom_needs_rebuild(t)) {
		xfg_table_bloom_rebuild(t);
		if (ctx->ndev)
			err = push_bloom(ctx, mi, -1);
	}
out:
	pthread_mutex_unlock(&ctx->lock);
	return err;
}

int xfg_map_get_next_key(xfg_ctx *ctx, int map, const void *key, void *next_key)
{
	int err = 0;
	if (!ctx || !next_key || keylen_of(map) < 0)
		return -EINVAL;
	if (map == XFG_MAP_PORTS) {
		/* BPF array semantics: next index; a missing/invalid key restarts at 0 */
		uint32_t k = 0;
		if (key) {
			memcpy(&k, key, 4);
			if (k >= XFG_PORT_MAP_ENTRIES)
				k = 0;
			else if (k + 1 >= XFG_PORT_MAP_ENTRIES)
				return -ENOENT;
			else
				k++;
		}
		memcpy(next_key, &k, 4);
		return 0;
	}
	pthread_mutex_lock(&ctx->lock);
	const struct xfg_table *t = &ctx->t[map - 1];
	int64_t after = -1;
	if (key)
		after = xfg_table_find(t, key); /* BPF htab: a missing key restarts at the first */
	int64_t s = xfg_table_next_slot(t, after);
	if (s < 0)
		err = -ENOENT;
	else
		err = xfg_table_slot_key(t, (uint64_t)s, next_key);
	pthread_mutex_unlock(&ctx->lock);
	return err;
}

int64_t xfg_map_count(xfg_ctx *ctx, int map)
{
	if (!ctx || keylen_of(map) < 0)
		return -EINVAL;
	if (map == XFG_MAP_PORTS)
		return ctx->port_count;
	return ctx->t[map - 1].count;
}

int64_t xfg_map_lookup_batch(xfg_ctx *ctx, int map, const void *keys, uint64_t n,
			     uint64_t *vals, uint8_t *present)
{
	int err = 0, kl = keylen_of(map);
	int64_t found = 0;
	if (!ctx || (!keys && n) || (!vals && n) || kl < 0)
		return -EINVAL;
	int nd = ctx->ndev ? ctx->ndev : 1;
	const struct xfg_table *t = map == XFG_MAP_PORTS ? NULL : &ctx->t[map - 1];
	size_t ns = t ? (size_t)t->nslots + 1 : XFG_PORT_MAP_ENTRIES;
	size_t fbytes = t ? xfg_table_img_bytes(t) : XFG_PORT_MAP_ENTRIES;
	uint8_t *flags = NULL;
	unsigned long long *hits = NULL;
	pthread_mutex_lock(&ctx->lock);
	if (ctx->ndev) {
		flags = malloc(fbytes * nd);
		hits = malloc(ns * 8 * nd);
		if (!flags || !hits) {
			err = -ENOMEM;
			goto out;
		}
		if (t && (err = qt_fold(ctx, map - 1)))
			goto out;
		for (int i = 0; i < ctx->ndev && !err; i++) {
			struct xfg_dev *d = &ctx->dev[i];
			const void *fsrc = t ? (const void *)d->m[map - 1].buckets : (const void *)d->port_flags;
			const unsigned long long *hsrc =
				t ? hits_view(ctx, d, map - 1)
				  : (ctx->reduced ? d->red_port_hits : d->port_hits);
			err = dev_read(d, flags + fbytes * i, fsrc, fbytes);
			if (!err)
				err = dev_read(d, hits + ns * i, hsrc, ns * 8);
		}
		if (err)
			goto out;
	}
	for (uint64_t i = 0; i < n; i++) {
		const uint8_t *k = (const uint8_t *)keys + (size_t)kl * i;
		int64_t s;
		if (!t) {
			uint32_t pk;
			s = port_key(k, &pk) ? -1 : (int64_t)pk;
		} else {
			s = xfg_table_find(t, k);
		}
		if (present)
			present[i] = s >= 0;
		for (int d = 0; d < nd; d++) {
			uint64_t v = 0;
			if (s >= 0) {
				if (!ctx->ndev) {
					v = t ? ctx->host_vals[map - 1][s] : ctx->host_port_vals[s];
				} else {
					uint8_t f = t ? flags[fbytes * d + xfg_table_flag_off(t, s)]
						      : flags[fbytes * d + s];
					v = (hits[ns * d + s] << XFG_COUNTER_SHIFT) | f;
				}
			}
			vals[i * nd + d] = v;
		}
		found += s >= 0;
	}
out:
	free(flags);
	free(hits);
	pthread_mutex_unlock(&ctx->lock);
	return err ? err : found;
}

/* vals[i] on every device (percpu = 0) or vals[i * nvals + d] (percpu = 1). */
static int update_batch(xfg_ctx *ctx, int map, const void *keys, const uint64_t *vals,
			uint64_t n, int percpu)
{
	int err = 0, kl = keylen_of(map);
	if (!ctx || (!keys && n) || (!vals && n) || kl < 0)
		return -EINVAL;
	const int nv = ctx->ndev ? ctx->ndev : 1;
#define VAL(i, d) (percpu ? vals[(i) * (uint64_t)nv + (d)] : vals[i])
	if (map == XFG_MAP_PORTS) {
		uint64_t v[64];
		uint64_t *vv = ctx->ndev > 64 ? calloc(ctx->ndev, 8) : v;
		if (!vv)
			return -ENOMEM;
		for (uint64_t i = 0; i < n && !err; i++) {
			for (int d = 0; d < nv; d++)
				vv[d] = VAL(i, d);
			err = xfg_map_update(ctx, map, (const uint8_t *)keys + 4 * i, vv);
		}
		if (vv != v)
			free(vv);
		return err;
	}
	pthread_mutex_lock(&ctx->lock);
	ctx->reduced = 0;
	int mi = map - 1;
	struct xfg_table *t = &ctx->t[mi];
	size_t ns = (size_t)t->nslots + 1, ib = xfg_table_img_bytes(t);
	uint8_t *img = NULL;           /* per-device bucket images */
	unsigned long long *hits = NULL;
	int nd = ctx->ndev;
	int fresh = t->count == 0;     /* nothing on the devices worth preserving */

	if (nd) {
		img = malloc(ib * nd);
		hits = malloc(ns * 8 * nd);
		if (!img || !hits) {
			err = -ENOMEM;
			goto out;
		}
		if ((err = qt_fold(ctx, mi)))
			goto out;
		for (int i = 0; i < nd && !err; i++) {
			struct xfg_dev *d = &ctx->dev[i];
			if (!fresh) {
				err = dev_read(d, img + ib * i, d->m[mi].buckets, ib);
				if (!err)
					err = dev_read(d, hits + ns * i, d->m[mi].hits, ns * 8);
			} else {
				memset(img + ib * i, 0, ib);
				memset(hits + ns * i, 0, ns * 8);
			}
		}
		if (err)
			goto out;
	}
	for (uint64_t i = 0; i < n; i++) {
		const uint8_t *k = (const uint8_t *)keys + (size_t)kl * i;
		int64_t s = xfg_table_find(t, k);
		if (s < 0)
			s = xfg_table_insert(t, k, NULL, NULL, NULL);
		if (s < 0) {
			err = (int)s;
			break;
		}
		uint8_t any = 0, all = 63;
		for (int d = 0; d < nv; d++) {
			any |= VAL(i, d) & 63;
			all &= VAL(i, d) & 63;
		}
		flags_note(ctx, mi, (uint64_t)s, any, all, 0);
		if (nd) {
			for (int d = 0; d < nd; d++) {
				img[ib * d + xfg_table_flag_off(t, s)] = VAL(i, d) & 63;
				hits[ns * d + s] = VAL(i, d) >> XFG_COUNTER_SHIFT;
			}
		} else {
			ctx->host_vals[mi][s] = VAL(i, 0);
		}
	}
#undef VAL
	/* merge host keys + meta into each device image (flags stay per device)
	 * and upload; also on partial failure: keys inserted so far stay */
	for (int i = 0; i < nd; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		uint8_t *di = img + ib * i;
		for (uint64_t b = 0; b <= t->nbuckets; b++) {
			memcpy(di + b * XFG_BUCKET_BYTES, t->img + b * XFG_BUCKET_BYTES, XFG_KEY_AREA);
			memcpy(di + b * XFG_BUCKET_BYTES + XFG_META_OFF,
			       t->img + b * XFG_BUCKET_BYTES + XFG_META_OFF, 4);
		}
		int e2 = dev_write(d, d->m[mi].buckets, di, ib);
		if (!e2)
			e2 = dev_write(d, d->m[mi].hits, hits + ns * i, ns * 8);
		if (!e2)
			e2 = dev_write(d, d->m[mi].bloom, t->bloom, (size_t)t->bloom_words * 4);
		if (e2 && !err)
			err = e2;
	}
out:
	free(img);
	free(hits);
	pthread_mutex_unlock(&ctx->lock);
	return err;
}

int xfg_map_update_batch(xfg_ctx *ctx, int map, const void *keys, const uint64_t *vals,
			 uint64_t n)
{
	return update_batch(ctx, map, keys, vals, n, 0);
}

int xfg_map_update_batch_percpu(xfg_ctx *ctx, int map, const void *keys, const uint64_t *vals,
				uint64_t n)
{
	return update_batch(ctx, map, keys, vals, n, 1);
}

/* ------------------------------------------------------------------ classify */
/* Device scratch buffer of at least @bytes (grown on demand; the old one may
 * still be in use by a launch queued on the device stream: wait for it). */
static int scratch(struct xfg_dev *d, void **p, uint64_t *have, uint64_t bytes)
{
	if (bytes <= *have)
		return 0;
	int err = hip_err(hipStreamSynchronize(d->stream));
	if (err)
		return err;
	hipFree(*p);
	*p = NULL;
	*have = 0;
	err = hip_err(hipMalloc(p, bytes));
	if (!err)
		*have = bytes;
	return err;
}

/* Rebuild a device's LDS port image from its flag bytes (d->lock held): the
 * open-addressed table (linear probing from xfg_port_slot()) when at most
 * XFG_PORT_TAB_MAX ports carry flags, else the nibble map of every port's
 * low 4 flag bits (the only ones CHECK_MAP can test). */
static int port_tab_refresh_locked(struct xfg_dev *d)
{
	uint32_t tab[XFG_PORT_TAB];
	uint32_t n = 0, disp = 0;
	if (!d->port_tab_dirty)
		return 0;
	memset(tab, 0, sizeof(tab));
	for (uint32_t k = 0; k < XFG_PORT_MAP_ENTRIES; k++) {
		if (!d->port_flags_h[k])
			continue;
		if (++n > XFG_PORT_TAB_MAX)
			break;
		uint32_t sl = xfg_port_slot(k), dd = 0;
		while (tab[sl]) {
			sl = (sl + 1) & (XFG_PORT_TAB - 1);
			dd++;
		}
		tab[sl] = ((uint32_t)d->port_flags_h[k] << 16) | k;
		if (dd > disp)
			disp = dd;
	}
	d->port_tab_ok = n <= XFG_PORT_TAB_MAX;
	d->port_tab_disp = disp;
	d->port_tab_dirty = 0;
	if (d->port_tab_ok)
		return dev_write(d, d->port_tab, tab, sizeof(tab));
	uint32_t *nib = calloc(XFG_PORT_NIB_WORDS, 4);
	if (!nib)
		return -ENOMEM;
	for (uint32_t k = 0; k < XFG_PORT_MAP_ENTRIES; k++)
		nib[k >> 3] |= (uint32_t)(d->port_flags_h[k] & 15) << ((k & 7) * 4);
	int err = dev_write(d, d->port_nib, nib, XFG_PORT_NIB_WORDS * 4);
	free(nib);
	return err;
}

static int port_tab_refresh(struct xfg_dev *d)
{
	/* (under the device lock: launch_batch reads the image's kind and
	 * displacement there; lock order ctx->lock, then d->lock) */
	pthread_mutex_lock(&d->lock);
	int err = port_tab_refresh_locked(d);
	pthread_mutex_unlock(&d->lock);
	return err;
}

/* Bring the quotient index of the IPv4 map up to date for lookups of mask
 * @live (ctx->lock held): rebuild the host image when the map changed, then
 * upload it to @d when its copy is older (under d->lock: launch_batch reads
 * the index's parameters there). */
static int qt_refresh(xfg_ctx *ctx, struct xfg_dev *d, uint32_t live)
{
	int err = 0;
	if (ctx->qt_dirty || !ctx->qt_gen || ctx->qt.live != live) {
		if ((err = xfg_qt_build(&ctx->qt, &ctx->t[0], ctx->flag_or[0], live,
					ctx->t[0].seed ^ 0x51ed2701u)))
			return err;
		ctx->qt_dirty = 0;
		if (!++ctx->qt_gen)
			ctx->qt_gen = 1;
	}
	if (d->qt_gen == ctx->qt_gen)
		return 0;
	const uint64_t ib = (uint64_t)ctx->qt.nimg * (1ull << ctx->qt.bits) * XFG_QT_BUCKET;
	const uint64_t tb = (uint64_t)ctx->qt.nimg * ctx->qt.nslots * 4;
	pthread_mutex_lock(&d->lock);
	if (!(err = qt_fold_locked(d)) &&   /* (through the index being replaced) */
	    !(err = scratch(d, (void **)&d->qt_img, &d->qt_img_bytes, ib)) &&
	    !(err = scratch(d, (void **)&d->qt_trans, &d->qt_trans_bytes, tb)) &&
	    !(err = dev_write(d, d->qt_img, ctx->qt.img, ib)) &&
	    !(err = dev_write(d, d->qt_trans, ctx->qt.trans, tb))) {
		d->qt_gen = ctx->qt_gen;
		d->qt_bits = ctx->qt.bits;
		d->qt_seed = ctx->qt.seed;
		d->qt_live = ctx->qt.live;
		d->qt_nimg = ctx->qt.nimg;
		d->qt_n = ctx->qt.nimg * ctx->qt.nslots;
	}
	pthread_mutex_unlock(&d->lock);
	return err;
}

/* The Ethernet map as the Ethernet-key kernel's key table (ctx->lock held):
 * rebuilt on the host after an edit, then uploaded to @d when its copy is
 * older.  A key at home xfg_ek_home, linear probing; slots
 * at least twice the keys.  ek_ok 0 (the generic kernel instead): more than
 * XFG_EK_MAX_KEYS keys, or a flag byte that differs between devices. */
static int ek_refresh(xfg_ctx *ctx, struct xfg_dev *d)
{
	int err = 0;
	const struct xfg_table *t = &ctx->t[2];
	if (!ctx->ek_gen || ctx->ek_seen != ctx->ek_edits) {
		ctx->ek_seen = ctx->ek_edits;
		if (!++ctx->ek_gen)
			ctx->ek_gen = 1;
		ctx->ek_ok = t->count <= XFG_EK_MAX_KEYS && !ctx->flag_cnt[2][7];
		if (!ctx->ek_ok)
			return 0;
		uint32_t sl = 64;
		while (sl < 2 * t->count)
			sl *= 2;
		memset(ctx->ek_host, 0, (size_t)sl * 16);
		ctx->ek_slots = sl;
		ctx->ek_disp = 0;
		for (int64_t s = xfg_table_next_slot(t, -1); s >= 0; s = xfg_table_next_slot(t, s)) {
			uint8_t k[8] = { 0 };
			if (xfg_table_slot_key(t, (uint64_t)s, k))
				continue;
			uint32_t lo, hi = k[4] | (uint32_t)k[5] << 8;
			memcpy(&lo, k, 4);
			uint32_t e = xfg_ek_home(lo, hi, t->seed, (uint32_t)__builtin_ctz(sl)), dsp = 0;
			while (ctx->ek_host[4 * e + 3] & XFG_EK_VALID) {
				e = (e + 1) & (sl - 1);
				dsp++;
			}
			ctx->ek_host[4 * e] = lo;
			ctx->ek_host[4 * e + 1] = hi;
			ctx->ek_host[4 * e + 2] = (uint32_t)s;
			ctx->ek_host[4 * e + 3] = XFG_EK_VALID | (ctx->flag_or[2][s] & 63);
			if (dsp > ctx->ek_disp)
				ctx->ek_disp = dsp;
		}
	}
	if (!ctx->ek_ok || d->ek_gen == ctx->ek_gen)
		return 0;
	pthread_mutex_lock(&d->lock);
	if (!(err = scratch(d, (void **)&d->ek_img, &d->ek_img_bytes, (uint64_t)XFG_EK_SLOTS_MAX * 16)) &&
	    !(err = dev_write(d, d->ek_img, ctx->ek_host, (size_t)ctx->ek_slots * 16))) {
		d->ek_gen = ctx->ek_gen;
		d->ek_slots = ctx->ek_slots;
		d->ek_disp = ctx->ek_disp;
	}
	pthread_mutex_unlock(&d->lock);
	return err;
}

/* One classify call between its two lock sections: the kernel arguments
 * the snapshot fills (the plan's follow in launch_batch) and the plan's
 * input. */
struct launch {
	struct xfg_kargs a;
	struct xfg_plan_in in;
	struct xfg_knobs knobs;
};

#ifdef XFG_DIAG
/* The measurement knobs (xfg_plan.h) from the environment, at every launch. */
static const struct xfg_knobs *knobs_read(struct xfg_knobs *k)
{
	xfg_knobs_init(k);
	for (const char *const *n = xfg_knob_names; *n; n++) {
		const char *v = getenv(*n);
		if (v)
			xfg_knobs_set(k, *n, v);
	}
	return k;
}
#else
#define knobs_read(k) NULL
#endif

/* Under ctx->lock: the census and the table descriptors as the batch's
 * launch will see them, and the device's images the plan asks for brought
 * up to date.  @db: the AF_XDP descriptors of the batch (@b then carries the
 * UMEM and the count, no lengths and no stride), or NULL; @hwin: a
 * header-window batch of the host path. */
static int snapshot(xfg_ctx *ctx, struct xfg_dev *d, const struct xfg_batch *b,
		    const struct xfg_desc_batch *db, uint8_t *verdicts, int hwin, struct launch *l)
{
	struct xfg_kargs *a = &l->a;
	struct xfg_plan_in *in = &l->in;
	memset(a, 0, sizeof(*a));
	memset(in, 0, sizeof(*in));
	pthread_mutex_lock(&ctx->lock);
	ctx->reduced = 0;
	int err = port_tab_refresh(d);
	if (err)
		goto out;
	struct xfg_tdesc *td[NMAPS_HASH] = { &a->t4, &a->t6, &a->te };
	uint64_t gb = 0;
	for (int i = 0; i < NMAPS_HASH; i++) {
		xfg_table_desc(&ctx->t[i], td[i]);
		td[i]->buckets = d->m[i].buckets;
		td[i]->bloom = d->m[i].bloom;
		td[i]->hits = d->m[i].hits;
		td[i]->fmask = census_mask(ctx->flag_cnt[i]);
		a->gbase[i] = (uint32_t)gb;
		gb += (uint64_t)ctx->t[i].nslots + 1;
		in->map[i].count = td[i]->count;
		in->map[i].fmask = td[i]->fmask;
		in->map[i].bloom_words = td[i]->bloom_words;
		in->map[i].nslots = td[i]->nslots;
	}
	a->gbase[3] = (uint32_t)gb;
	a->port_fmask = census_mask(ctx->port_flag_cnt);
	a->port_hits = d->port_hits;
	a->port_count = ctx->port_count;
	a->port_nib = d->port_nib;
	a->stats = d->stats;
	a->data = b->data;
	a->offsets = b->offsets;
	a->lens = b->lens;
	a->n = b->count;
	a->stride = b->stride;
	a->lens_u16 = b->lens_u16;
	a->verdicts = verdicts;
	a->hwin = hwin;
	if (db) {
		a->descs = db->descs;
		a->desc_mask = db->mask;
		a->desc_first = db->first;
	}
	in->feat = ctx->prog_features;
	in->flags_differ4 = ctx->flag_cnt[0][7];
	in->port_count = ctx->port_count;
	in->ctx_window = ctx->window;
	in->qt_min_keys = ctx->qt_min_keys;
	in->descs_min = ctx->descs_min;
	in->n = b->count;
	in->stride = b->stride;
	in->offsets = b->offsets != NULL;
	in->aligned16 = !((uintptr_t)b->data & 15);
	in->descs = db != NULL;
	in->hwin = hwin;
	in->ncu = d->ncu;
	in->occ = d->occ;
	in->thr = d->thr;
	in->knobs = knobs_read(&l->knobs);
	if (in->knobs) {
		a->diag = in->knobs->diag_mask;
		a->tstamp = (unsigned long long *)(uintptr_t)in->knobs->tstamp;
		if (in->knobs->empty) {
			a->t4.count = a->t6.count = a->te.count = 0;
			a->port_count = 0;
		}
	}
	struct xfg_wants w;
	xfg_plan_wants(in, &w);
	if (w.ek) {
		if ((err = ek_refresh(ctx, d)))
			goto out;
		in->ek_ok = ctx->ek_ok;
		xfg_plan_wants(in, &w);
	}
	if (w.qt_live)
		err = qt_refresh(ctx, d, w.qt_live);
out:
	pthread_mutex_unlock(&ctx->lock);
	return err;
}

/* Work on the device's own stream between a caller's: after what @user (a
 * caller's stream; NULL or the device's own: nothing to order) holds ... */
static int stream_enter(struct xfg_dev *d, void *user)
{
	if (!user || user == (void *)d->stream)
		return 0;
	int err = hip_err(hipEventRecord(d->ev_user, (hipStream_t)user));
	return err ? err : hip_err(hipStreamWaitEvent(d->stream, d->ev_user, 0));
}

/* ... and @user's later work after it. */
static int stream_leave(struct xfg_dev *d, void *user)
{
	if (!user || user == (void *)d->stream)
		return 0;
	int err = hip_err(hipEventRecord(d->ev_done, d->stream));
	return err ? err : hip_err(hipStreamWaitEvent((hipStream_t)user, d->ev_done, 0));
}

/* classify launches on the device's own stream (every classify of a device
 * is serialised there), ordered after and before @user (a caller's stream,
 * or NULL).  Under the device lock: the plan from the device's images in
 * stream order at this launch, the per-launch scratch (hit log, deferred
 * lists) sized and used, so concurrent callers never see a buffer being
 * replaced. */
static int launch_batch(xfg_ctx *ctx, struct xfg_dev *d, struct launch *l, void *user, int iters)
{
	int err = 0;
	struct xfg_kargs *a = &l->a;
	struct xfg_plan_in *in = &l->in;
	struct xfg_plan p;
	pthread_mutex_lock(&d->lock);
	/* (another caller's refresh may have rewritten the images since the
	 * snapshot; both hold d->lock for that) */
	in->port_tab_ok = d->port_tab_ok;
	in->qt_n = d->qt_n;
	in->qt_live = d->qt_live;
	in->qt_nimg = d->qt_nimg;
	in->qt_bits = d->qt_bits;
	in->ek_slots = d->ek_slots;
	xfg_plan(in, &p);
	const uint64_t grid = p.grid;
	a->port_tab = d->port_tab_ok ? d->port_tab : NULL;
	a->port_tab_disp = d->port_tab_disp;
	a->window = p.window;
	a->pipe = p.pipe;
	a->dense = p.dense;
	a->km = p.km;
	a->v6d = p.v6d;
	a->v6p = p.v6p;
	a->split = p.split;
	a->bloom_off = p.bloom_off;
	a->grid_parse = p.grid_parse;
	a->dcnt = p.dcnt;
	a->bl_lds = p.bl_lds;
	memcpy(a->bl_off, p.bl_off, sizeof(a->bl_off));
	a->qt_dyn = p.qt_dyn;
	if (p.use_ek) {
		a->ek = d->ek_img;
		a->ek_slots = d->ek_slots;
		a->ek_disp = d->ek_disp;
	}
	if (p.use_qt) {
		a->qt = d->qt_img;
		a->qt_trans = d->qt_trans;
		a->qt_bits = d->qt_bits;
		a->qt_seed = d->qt_seed;
		a->qt_live = d->qt_live;
		a->qt_n = d->qt_n;
		/* the second (src) lookup's image and its slots' offset: the same
		 * image at offset 0 when one serves both directions */
		a->qt_base = d->qt_nimg == 2 ? d->qt_n / 2 : 0;
		a->qt2 = d->qt_img + (uint64_t)a->qt_base * 2 / 4;
		/* its QT-order counts (zeroed when (re)allocated; a resize only
		 * follows a fold: qt_refresh) */
		const uint64_t had = d->qt_hits_bytes;
		if ((err = scratch(d, (void **)&d->qt_hits, &d->qt_hits_bytes, p.bytes.qt_hits)))
			goto out;
		if (d->qt_hits_bytes != had &&
		    (err = hip_err(hipMemsetAsync(d->qt_hits, 0, d->qt_hits_bytes, d->stream))))
			goto out;
		a->qt_hits = d->qt_hits;
		a->qt_hitx = d->qt_hits + d->qt_n;
	}
	if (p.split) {
		if ((err = scratch(d, (void **)&d->rec, &d->rec_bytes, p.bytes.rec)))
			goto out;
		a->rec_ka = d->rec;
		a->rec_port = d->rec + a->n;
		a->rec_kb = p.rec_both ? d->rec + 2 * a->n : NULL;
	}
	if (p.bytes.defer) {
		if ((err = scratch(d, (void **)&d->defer, &d->defer_bytes, p.bytes.defer)))
			goto out;
		a->defer = d->defer;
		a->defer_cap = p.defer_cap;
	}
	if (p.defer_sep) {
		if ((err = scratch(d, (void **)&d->defer_n, &d->defer_n_bytes, p.bytes.defer_n)))
			goto out;
		a->defer_n = d->defer_n;
		a->defer_nsrc = p.defer_nsrc;
		a->defer_sep = 1;
		a->defer_grid = p.defer_grid;
	}
	/* logs pending from earlier launches: counted first unless this one
	 * appends to them -- or, in the count wave's mode, counts them (the
	 * same shape, the same counts) */
	const int append = p.logs && p.K > 1 && d->log_pend && d->log_grid == grid &&
			   d->log_args.pcap == p.pcap && d->log_args.pslices == p.K * grid &&
			   d->log_args.log_span == p.log_span && d->log_args.pwide == p.pwide &&
			   d->log_args.qt_hits == a->qt_hits && d->log_args.qt_n == a->qt_n &&
			   d->log_cw == (uint32_t)p.cw;
	if (d->log_pend && !append && (err = log_flush_locked(d)))
		goto out;
	if (p.logs) {
		if ((err = scratch(d, (void **)&d->tlog, &d->tlog_bytes, p.bytes.tlog)) ||
		    (err = scratch(d, (void **)&d->pbuf, &d->pbuf_bytes, p.bytes.pbuf)) ||
		    (err = scratch(d, (void **)&d->pfill, &d->pfill_bytes, p.bytes.pfill)))
			goto out;
		a->tlog = p.bytes.tlog ? d->tlog : NULL;
		a->pbuf = d->pbuf;
		a->pfill = d->pfill;
		a->pcap = p.pcap;
		a->pslices = p.K * (uint32_t)grid;
		a->pslice0 = 0;
		a->pcount = (uint32_t)grid;
		a->log_hist = p.log_hist;
		a->log_span = p.log_span;
		a->pwide = p.pwide;
	}
	if ((err = stream_enter(d, user)))
		goto out;
	if (a->qt_hits && iters > 0)
		d->qt_pending = 1;
	/* classify, then its hit log's count kernel, on the device stream (a
	 * count kernel on a second stream, overlapped with the next classify,
	 * shares the CUs and slowed the classify more than it hid:
	 * profiles/archive/r04_s11_count_overlap.log) */
	/* (a fold before a 32-bit QT-order count could run out of room) */
	const uint64_t fold_at = in->knobs && in->knobs->qt_fold_at ? in->knobs->qt_fold_at : 0xffffffffull;
	for (int i = 0; i < iters && !err; i++) {
		if (a->qt_hits) {
			if (d->qt_pk + a->n > fold_at && (err = qt_fold_queued(d)))
				break;
			d->qt_pk += a->n;
		}
		a->cw_n = 0;
		a->pfirst = 0;
		if (a->pbuf && p.cw) {
			/* the pending launch's set, counted by this launch's count
			 * wave (or, with none pending, none); this launch's log
			 * into the other set */
			if (d->log_pend) {
				a->cw_n = (uint32_t)grid;
				a->cw_s0 = d->log_first;
			}
			a->pslice0 = d->log_pend && !d->log_first ? (uint32_t)grid : 0u;
		} else if (a->pbuf && p.K > 1) {
			a->pslice0 = d->log_pend * (uint32_t)grid;
		}
		err = xfg_launch_classify(ctx->prog_features, a, (unsigned)grid, d->stream);
		if (!err && a->pbuf && p.cw) {
			d->log_args = *a;
			d->log_grid = (uint32_t)grid;
			d->log_pend = 1;
			d->log_first = a->pslice0;
			d->log_cw = 1;
		} else if (!err && a->pbuf && p.K > 1) {
			if (!d->log_pend)
				d->log_first = 0;
			d->log_args = *a;
			d->log_grid = (uint32_t)grid;
			d->log_cw = 0;
			if (++d->log_pend == p.K)
				err = log_flush_locked(d);
		} else if (!err) {
			err = xfg_launch_log_count(a, d->stream);
		}
	}
	if (!err)
		d->last_kind = p.kind;
	if (!err)
		err = stream_leave(d, user);
out:
	pthread_mutex_unlock(&d->lock);
	return err;
}

/* the device argument of an entry point (@ctx checked) */
static int dev_check(const xfg_ctx *ctx, int dev)
{
	if (!ctx->ndev)
		return -ENODEV;
	if (dev < 0 || dev >= ctx->ndev)
		return -EINVAL;
	return 0;
}

/* what the entry points refuse of a batch's own fields ... */
static int batch_bad(const struct xfg_batch *b)
{
	if (b->count && (!b->data || !b->lens))
		return 1;
	if (!b->offsets && b->count && (b->stride == 0 || (b->stride & 15)))
		return 1;
	return ((uintptr_t)b->data & 15) != 0;
}

/* ... and of a descriptor batch's that is not empty */
static int descs_bad(const struct xfg_desc_batch *db)
{
	return !db->umem || !db->descs || ((uintptr_t)db->descs & 7) || (db->mask & (db->mask + 1u));
}

static int check_batch(xfg_ctx *ctx, int dev, const struct xfg_batch *b, const void *verdicts)
{
	if (!ctx || !b || (!verdicts && b->count))
		return -EINVAL;
	const int err = dev_check(ctx, dev);
	if (err)
		return err;
	return batch_bad(b) ? -EINVAL : 0;
}

/* argument checks of the descriptor entry points; 1: an empty batch */
static int check_descs(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db, const void *verdicts)
{
	if (!ctx || !db || (!verdicts && db->count))
		return -EINVAL;
	const int err = dev_check(ctx, dev);
	if (err)
		return err;
	if (!db->count)
		return 1;
	return descs_bad(db) ? -EINVAL : 0;
}

/* The four entry points' body, their arguments checked: @iters launches of
 * @b, or of the descriptor batch @db; with @avg_ms between two events on
 * the device's stream, the logs still pending counted inside the timed
 * region (the iterations' work is complete when ev1 fires). */
static int classify(xfg_ctx *ctx, int dev, const struct xfg_batch *b, const struct xfg_desc_batch *db,
		    uint8_t *verdicts, void *stream, int iters, double *avg_ms)
{
	struct xfg_dev *d = &ctx->dev[dev];
	struct xfg_batch umem;
	struct launch l;
	float ms = 0;
	if (db) {
		umem = (struct xfg_batch){ db->umem, NULL, NULL, db->count, 0, 0 };
		b = &umem;
	}
	int err = snapshot(ctx, d, b, db, verdicts, 0, &l);
	if (err)
		return err;
	HIPCHK(hipSetDevice(d->ordinal));
	if (!avg_ms)
		return launch_batch(ctx, d, &l, stream, iters);
	HIPCHK(hipEventRecord(d->ev0, d->stream));
	if ((err = launch_batch(ctx, d, &l, NULL, iters)))
		goto fail;
	pthread_mutex_lock(&d->lock);
	err = log_flush_locked(d);
	pthread_mutex_unlock(&d->lock);
	if (err)
		goto fail;
	HIPCHK(hipEventRecord(d->ev1, d->stream));
	HIPCHK(hipEventSynchronize(d->ev1));
	HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
	*avg_ms = ms / iters;
fail:
	return err;
}

int xfg_classify(xfg_ctx *ctx, int dev, const struct xfg_batch *b, uint8_t *verdicts,
		 void *stream)
{
	int err = check_batch(ctx, dev, b, verdicts);
	if (err || !b->count)
		return err;
	return classify(ctx, dev, b, NULL, verdicts, stream, 1, NULL);
}

int xfg_classify_descs(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
		       uint8_t *verdicts, void *stream)
{
	int err = check_descs(ctx, dev, db, verdicts);
	if (err)
		return err < 0 ? err : 0;
	return classify(ctx, dev, NULL, db, verdicts, stream, 1, NULL);
}

int xfg_classify_descs_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
			     uint8_t *verdicts, int iters, double *avg_ms)
{
	int err = check_descs(ctx, dev, db, verdicts);
	if (err < 0)
		return err;
	if (iters < 1 || !avg_ms || err)   /* (an empty batch has no time) */
		return -EINVAL;
	return classify(ctx, dev, NULL, db, verdicts, NULL, iters, avg_ms);
}

int xfg_classify_timed(xfg_ctx *ctx, int dev, const struct xfg_batch *b, uint8_t *verdicts,
		       int iters, double *avg_ms)
{
	int err = check_batch(ctx, dev, b, verdicts);
	if (err)
		return err;
	if (iters < 1 || !avg_ms)
		return -EINVAL;
	return classify(ctx, dev, b, NULL, verdicts, NULL, iters, avg_ms);
}

/* Room for @words status words in the device's tile status buffer (d->lock
 * held, the device current): shared by every launch that goes through
 * scratch_launch() or staged_run(), which run one after the other on the
 * device's stream and each zero the words they use first. */
static int cstatus_room(struct xfg_dev *d, uint64_t words)
{
	int err = 0;
	if (words <= d->cstatus_cap)
		return 0;
	HIPCHK(hipStreamSynchronize(d->stream));   /* the old buffer may be in use */
	hipFree(d->cstatus);
	d->cstatus = NULL;
	d->cstatus_cap = 0;
	HIPCHK(hipMalloc((void **)&d->cstatus, words * 8));
	d->cstatus_cap = words;
fail:
	return err;
}

/* One launch over the device's status scratch (@words of it), on the device's
 * own stream between @stream's earlier and later work: two such launches never
 * overlap on a device, whatever streams their callers pass.  @launch (d->lock
 * held, the device current) points its kernel's state words at d->cstatus and
 * launches on d->stream with four workgroups a CU, all of them resident.  An
 * empty batch (@zero: the call's counts, @zero_bytes of them) needs no
 * scratch: the counts are zeroed on the caller's stream itself.  What else
 * @launch allocates (the compaction ticket, the capture scan's per-record
 * scratch) it allocates with the stream entered: a failed allocation costs
 * the caller's stream one event wait.  Once the device's stream was entered
 * it is left too, also after a failed launch (the caller's stream behind
 * whatever was queued); the first error is returned. */
static int scratch_launch(struct xfg_dev *d, void *stream, void *zero, size_t zero_bytes,
			  uint64_t words, int (*launch)(struct xfg_dev *d, unsigned grid, void *arg),
			  void *arg)
{
	int err = 0;
	pthread_mutex_lock(&d->lock);
	HIPCHK(hipSetDevice(d->ordinal));
	if (zero) {
		HIPCHK(hipMemsetAsync(zero, 0, zero_bytes, stream ? (hipStream_t)stream : d->stream));
		goto fail;
	}
	if ((err = cstatus_room(d, words)) || (err = stream_enter(d, stream)))
		goto fail;
	err = launch(d, (unsigned)d->ncu * 4, arg);
	const int e2 = stream_leave(d, stream);
	err = err ? err : e2;
fail:
	pthread_mutex_unlock(&d->lock);
	return err;
}

/* The calls that classify in stages (multi-buffer batches, chained stages,
 * many sockets) are one sequence, staged_run()'s: a pre-pass over the caller's
 * records that leaves a plain descriptor array, its counts read back, the
 * array classified through classify(), and a post-pass that writes the
 * verdicts back over the records by index.  What differs is this job.  @pre
 * and @got run with d->lock held, the device current and its stream entered. */
struct staged {
	pthread_mutex_t *lock;  /* the call's outer lock: frags_lock, socks_lock */
	uint64_t words;         /* status words of d->cstatus the pre-pass uses */
	uint64_t n;             /* records fr_heads and fr_pv are sized for (0: neither) */
	uint32_t *idx;          /* their indices: the caller's, or NULL: fr_pkt, sized too
	                         * (@got may point it at what the post-pass reads instead) */
	uint8_t *verdicts;      /* the caller's verdict bytes */
	const void *umem;       /* classify(): the frames' base, */
	const void *descs;      /* their descriptors (NULL: fr_heads; @pre may set it) */
	uint64_t count;         /* and how many: from @got, or the caller's total */
	uint64_t back;          /* records the post-pass writes now, by the call's rule */
	int (*pre)(struct xfg_dev *d, struct staged *j);   /* launches on d->stream */
	/* optional: the state words copied back and waited for (the call's one
	 * host synchronisation), checked (-EIO), the caller's counts, @count, @back */
	int (*got)(struct xfg_dev *d, struct staged *j);
	/* optional (without it classify() writes @verdicts itself): fr_pv to
	 * @verdicts by @idx, @back records of them */
	int (*post)(const uint8_t *pv, const uint32_t *idx, uint8_t *verdicts, uint32_t n,
		    unsigned grid, void *stream);
	const void *arg;        /* the hooks': what the pre-pass reads, */
	void *out;              /* the caller's struct with its counts */
};

/* the time on the device's stream since ev0 was recorded, waited for */
static int ev_elapsed(struct xfg_dev *d, double *ms)
{
	float t = 0;
	int err = hip_err(hipEventRecord(d->ev1, d->stream));
	if (!err && !(err = hip_err(hipEventSynchronize(d->ev1))))
		err = hip_err(hipEventElapsedTime(&t, d->ev0, d->ev1));
	*ms = t;
	return err;
}

/* All of a staged call on the device's own stream, after @stream's earlier
 * work and before its later.  The outer lock keeps a second caller off the
 * scratch between the steps: d->lock itself is released around classify(),
 * which takes it.  @ms (the timed entry points): the three steps' durations,
 * each between two events and waited for.  Once the device's stream was
 * entered it is left too, whatever failed -- a hook, classify(), making the
 * device current again behind it (-EIO, unless classify() failed) -- with
 * d->lock held and the caller's stream behind whatever was queued; the first
 * error is returned. */
static int staged_run(xfg_ctx *ctx, int dev, struct staged *j, void *stream, double *ms)
{
	struct xfg_dev *d = &ctx->dev[dev];
	int err = 0, entered = 0;
	pthread_mutex_lock(j->lock);
	pthread_mutex_lock(&d->lock);
	HIPCHK(hipSetDevice(d->ordinal));
	if ((err = cstatus_room(d, j->words)) ||
	    (err = scratch(d, &d->fr_heads, &d->fr_heads_bytes, j->n * 16)) ||
	    (err = scratch(d, (void **)&d->fr_pv, &d->fr_pv_bytes, j->n)) ||
	    (!j->idx && (err = scratch(d, (void **)&d->fr_pkt, &d->fr_pkt_bytes, j->n * 4))))
		goto fail;
	if (!j->idx)
		j->idx = d->fr_pkt;
	if ((err = stream_enter(d, stream)))
		goto fail;
	entered = 1;
	if (ms)
		HIPCHK(hipEventRecord(d->ev0, d->stream));
	if ((err = j->pre(d, j)) || (ms && (err = ev_elapsed(d, &ms[0]))) ||
	    (j->got && (err = j->got(d, j))))
		goto fail;
	if (j->count) {
		const struct xfg_desc_batch hb = { j->umem, j->descs ? j->descs : d->fr_heads, 0,
						   0xffffffffu, j->count };
		uint8_t *pv = j->post ? d->fr_pv : j->verdicts;
		pthread_mutex_unlock(&d->lock);
		err = classify(ctx, dev, NULL, &hb, pv, NULL, 1, ms ? &ms[1] : NULL);
		pthread_mutex_lock(&d->lock);
		if (hipSetDevice(d->ordinal) != hipSuccess)
			err = err ? err : -EIO;
		if (err)
			goto fail;
	}
	if (j->post && j->back) {
		if (ms)
			HIPCHK(hipEventRecord(d->ev0, d->stream));
		if ((err = j->post(d->fr_pv, j->idx, j->verdicts, (uint32_t)j->back, (unsigned)d->ncu * 8,
				   d->stream)) ||
		    (ms && (err = ev_elapsed(d, &ms[2]))))
			goto fail;
	}
fail:
	if (entered) {
		const int e2 = stream_leave(d, stream);
		err = err ? err : e2;
	}
	pthread_mutex_unlock(&d->lock);
	pthread_mutex_unlock(j->lock);
	return err;
}

/* Verdict compaction (include/xdpfilter_gpu.h). */
struct compact_job {
	const uint8_t *verdicts;
	uint64_t n;
	uint32_t action;
	uint32_t *idx;
	uint64_t *count;
};

static int compact_go(struct xfg_dev *d, unsigned grid, void *arg)
{
	const struct compact_job *j = arg;
	int err = 0;
	if (!d->cticket)
		HIPCHK(hipMalloc((void **)&d->cticket, 4));
	err = xfg_launch_compact(j->verdicts, j->n, j->action, j->idx, (unsigned long long *)j->count,
				 d->cstatus, d->cticket, grid, d->stream);
fail:
	return err;
}

int xfg_compact(xfg_ctx *ctx, int dev, const uint8_t *verdicts, uint64_t n, uint32_t action,
		uint32_t *idx, uint64_t *count, void *stream)
{
	int err;
	if (!ctx || !count || (n && (!verdicts || !idx)) || action > 255 || n > 0xffffffffull)
		return -EINVAL;
	if ((err = dev_check(ctx, dev)))
		return err;
	struct compact_job j = { verdicts, n, action, idx, count };
	/* (an empty batch too: its count is zeroed by the launch function) */
	return scratch_launch(&ctx->dev[dev], stream, NULL, 0, xfg_compact_tiles(n), compact_go, &j);
}

/* a ring mask: 2^k - 1 (0xffffffff: a plain array) */
static int mask_ok(uint32_t mask)
{
	return !(mask & (mask + 1u));
}

/* AF_XDP egress (include/xdpfilter_gpu.h). */
static int egress_go(struct xfg_dev *d, unsigned grid, void *arg)
{
	struct xfg_egress_kargs *a = arg;
	a->state = d->cstatus;
	return xfg_launch_egress(a, grid, d->stream);
}

int xfg_ring_egress(xfg_ctx *ctx, int dev, const struct xfg_egress *e, const uint8_t *verdicts,
		    void *stream)
{
	int err;
	if (!ctx || !e || e->sz < sizeof(*e) || !e->counts || ((uintptr_t)e->counts & 7) ||
	    (e->flags & ~(XFG_EGRESS_SWAP_MACS | XFG_EGRESS_MULTIBUF)) || e->count > 0xffffffffull ||
	    (!e->tx_descs && !e->fill_addrs))
		return -EINVAL;
	if (!mask_ok(e->rx_mask) || !mask_ok(e->tx_mask) || !mask_ok(e->fill_mask))
		return -EINVAL;
	if (((uintptr_t)e->rx_descs & 7) || ((uintptr_t)e->tx_descs & 7) ||
	    ((uintptr_t)e->fill_addrs & 7) || ((uintptr_t)e->umem & 7))
		return -EINVAL;
	if ((e->tx_descs && (uint64_t)e->tx_mask + 1 < e->count) ||
	    (e->fill_addrs && (uint64_t)e->fill_mask + 1 < e->count))
		return -EINVAL;
	if ((e->flags & XFG_EGRESS_SWAP_MACS) && !e->umem)
		return -EINVAL;
	if (e->count && (!e->rx_descs || (e->tx_descs && !verdicts)))
		return -EINVAL;
	if ((err = dev_check(ctx, dev)))
		return err;
	struct xfg_egress_kargs a = {
		.umem = (e->flags & XFG_EGRESS_SWAP_MACS) ? e->umem : NULL,
		.rx = e->rx_descs, .tx = e->tx_descs, .fill = e->fill_addrs,
		.verdicts = verdicts, .counts = (unsigned long long *)e->counts,
		.rx_first = e->rx_first, .rx_mask = e->rx_mask,
		.tx_first = e->tx_first, .tx_mask = e->tx_mask,
		.fill_first = e->fill_first, .fill_mask = e->fill_mask,
		.n = (uint32_t)e->count,
		.swap_macs = !!(e->flags & XFG_EGRESS_SWAP_MACS),
		.multibuf = !!(e->flags & XFG_EGRESS_MULTIBUF),
	};
	return scratch_launch(&ctx->dev[dev], stream, e->count ? NULL : e->counts, 16,
			      XFG_EGRESS_STATE_WORDS(e->count), egress_go, &a);
}

/* Multi-buffer descriptor batches (include/xdpfilter_gpu.h), a staged call
 * under frags_lock: the head pass over the records, its packet and record
 * counts read back (the classify launch is planned from the packet count), the
 * packets' head records classified, and their verdicts spread over the records
 * of complete packets, if there are any. */
static int frags_pre(struct xfg_dev *d, struct staged *j)
{
	const struct xfg_desc_batch *db = j->arg;
	const struct xfg_frags_kargs a = {
		.rx = db->descs, .pkt_of = j->idx, .heads = d->fr_heads, .state = d->cstatus,
		.first = db->first, .mask = db->mask, .n = (uint32_t)j->n,
	};
	/* (four workgroups a CU: all of them resident) */
	return xfg_launch_frags_heads(&a, (unsigned)d->ncu * 4, d->stream);
}

static int frags_got(struct xfg_dev *d, struct staged *j)
{
	struct xfg_frags *fr = j->out;
	unsigned long long got[2] = { 0, 0 };
	const int err = dev_read(d, got, d->cstatus + 2, sizeof(got));
	if (err)
		return err;
	if (got[0] > j->n || got[1] > j->n || (got[0] != 0) != (got[1] != 0))
		return -EIO;
	fr->counts[0] = j->count = got[0];
	fr->counts[1] = j->back = got[1];
	fr->counts[2] = j->n - got[1];
	return 0;
}

static int frags_run(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db, struct xfg_frags *fr,
		     uint8_t *verdicts, void *stream, double *ms)
{
	if (!db || !fr || fr->sz < sizeof(*fr) || ((uintptr_t)fr->pkt_of & 3) ||
	    db->count > 0xffffffffull)
		return -EINVAL;
	int err = check_descs(ctx, dev, db, verdicts);
	if (err < 0)
		return err;
	fr->counts[0] = fr->counts[1] = fr->counts[2] = 0;
	if (ms)
		ms[0] = ms[1] = ms[2] = 0;
	if (err)   /* an empty batch */
		return 0;
	struct staged j = {
		.lock = &ctx->dev[dev].frags_lock, .words = XFG_FRAGS_STATE_WORDS(db->count),
		.n = db->count, .idx = fr->pkt_of, .verdicts = verdicts, .umem = db->umem,
		.pre = frags_pre, .got = frags_got, .post = xfg_launch_frags_spread,
		.arg = db, .out = fr,
	};
	return staged_run(ctx, dev, &j, stream, ms);
}

int xfg_classify_descs_frags(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
			     struct xfg_frags *fr, uint8_t *verdicts, void *stream)
{
	return frags_run(ctx, dev, db, fr, verdicts, stream, NULL);
}

int xfg_classify_descs_frags_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
				   struct xfg_frags *fr, uint8_t *verdicts, double ms[3])
{
	if (!ms)
		return -EINVAL;
	return frags_run(ctx, dev, db, fr, verdicts, NULL, ms);
}

/* A chained stage (include/xdpfilter_gpu.h) over @b or over @db, a staged
 * call: the select pass over the earlier stage's verdict bytes, the selected
 * count read back (the classify launch is planned from it), the selected
 * frames classified as a plain descriptor array over the batch's bytes, and
 * their verdicts scattered to the frames' own bytes, if any was selected.
 * Under frags_lock, whose scratch it uses (the heads' room for the
 * descriptors, the packet indices' for idx).  The argument checks come first
 * and the empty batch next, neither needing a device. */
static int chain_pre(struct xfg_dev *d, struct staged *j)
{
	struct xfg_chain_kargs a = *(const struct xfg_chain_kargs *)j->arg;   /* (the frames) */
	a.idx = j->idx;
	a.sel = d->fr_heads;
	a.state = d->cstatus;
	/* (four workgroups a CU: all of them resident) */
	return xfg_launch_chain_select(&a, (unsigned)d->ncu * 4, d->stream);
}

static int chain_got(struct xfg_dev *d, struct staged *j)
{
	struct xfg_chain *ch = j->out;
	unsigned long long got = 0;
	const int err = dev_read(d, &got, d->cstatus + 2, sizeof(got));
	if (err)
		return err;
	if (got > j->n)
		return -EIO;
	ch->counts[0] = j->count = j->back = got;
	ch->counts[1] = j->n - got;
	return 0;
}

static int chain_run(xfg_ctx *ctx, int dev, const struct xfg_batch *b,
		     const struct xfg_desc_batch *db, struct xfg_chain *ch, uint8_t *verdicts,
		     void *stream, double *ms)
{
	if (!ctx || (!b && !db) || !ch || ch->sz < sizeof(*ch) || ch->flags ||
	    ((uintptr_t)ch->idx & 3))
		return -EINVAL;
	const uint64_t n = db ? db->count : b->count;
	if (n > 0xffffffffull || (n && !verdicts) || (b ? batch_bad(b) : n && descs_bad(db)))
		return -EINVAL;
	/* (a frame's offset travels in a descriptor's 48-bit address field) */
	if (b && !b->offsets && n * b->stride > 1ull << 48)
		return -EINVAL;
	if (ms)
		ms[0] = ms[1] = ms[2] = 0;
	if (!n) {
		ch->counts[0] = ch->counts[1] = 0;
		return 0;
	}
	int err = dev_check(ctx, dev);
	if (err)
		return err;
	ch->counts[0] = 0;
	ch->counts[1] = n;
	if (!ch->chain_mask)
		return 0;
	struct xfg_chain_kargs a = {
		.verdicts = verdicts, .n = (uint32_t)n, .chain_mask = ch->chain_mask,
	};
	if (db) {
		a.descs = db->descs;
		a.first = db->first;
		a.mask = db->mask;
		a.form = XFG_CHAIN_F_DESCS;
	} else {
		a.offsets = b->offsets;
		a.lens = b->lens;
		a.stride = b->stride;
		a.form = b->lens_u16 ? XFG_CHAIN_F_LENS_U16 : 0;
	}
	struct staged j = {
		.lock = &ctx->dev[dev].frags_lock, .words = XFG_CHAIN_STATE_WORDS(n), .n = n,
		.idx = ch->idx, .verdicts = verdicts, .umem = db ? db->umem : b->data,
		.pre = chain_pre, .got = chain_got, .post = xfg_launch_chain_scatter,
		.arg = &a, .out = ch,
	};
	return staged_run(ctx, dev, &j, stream, ms);
}

int xfg_classify_chain(xfg_ctx *ctx, int dev, const struct xfg_batch *b, struct xfg_chain *ch,
		       uint8_t *verdicts, void *stream)
{
	return b ? chain_run(ctx, dev, b, NULL, ch, verdicts, stream, NULL) : -EINVAL;
}

int xfg_classify_descs_chain(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
			     struct xfg_chain *ch, uint8_t *verdicts, void *stream)
{
	return db ? chain_run(ctx, dev, NULL, db, ch, verdicts, stream, NULL) : -EINVAL;
}

int xfg_classify_descs_chain_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
				   struct xfg_chain *ch, uint8_t *verdicts, double ms[3])
{
	return db && ms ? chain_run(ctx, dev, NULL, db, ch, verdicts, NULL, ms) : -EINVAL;
}

/* A chained stage over a multi-buffer batch (include/xdpfilter_gpu.h), a
 * staged call under frags_lock: the record pass and the segment pass over the
 * records and the earlier stage's verdict bytes, the selected packets and
 * their records read back (the classify launch is planned from the packets),
 * the packets' head records classified as a plain descriptor array, and their
 * verdicts spread over all records by segment, if any packet was selected.
 * Its scratch is the frags calls' (the heads' room, the per-packet verdicts,
 * the packet indices' for idx) and the segment arrays, grown by the pre-pass
 * with the stream entered as the capture scan's are.  The argument checks come
 * first and the empty batch next, neither needing a device. */
static int frags_chain_pre(struct xfg_dev *d, struct staged *j)
{
	struct xfg_frags_chain_kargs a = *(const struct xfg_frags_chain_kargs *)j->arg;
	const int err = scratch(d, (void **)&d->fc_seg, &d->fc_seg_bytes, XFG_FRAGS_CHAIN_SEG_BYTES(j->n));
	if (err)
		return err;
	a.idx = j->idx;
	a.sel = d->fr_heads;
	a.seg = d->fc_seg;
	a.state = d->cstatus;
	/* (four workgroups a CU: all of them resident) */
	return xfg_launch_frags_chain_select(&a, (unsigned)d->ncu * 4, d->stream);
}

static int frags_chain_got(struct xfg_dev *d, struct staged *j)
{
	struct xfg_frags_chain *ch = j->out;
	unsigned long long got[2] = { 0, 0 };
	const int err = dev_read(d, got, d->cstatus + 2, sizeof(got));
	if (err)
		return err;
	/* (a packet has at least one record) */
	if (got[1] > j->n || got[0] > got[1] || (got[0] != 0) != (got[1] != 0))
		return -EIO;
	ch->counts[0] = j->count = got[0];
	ch->counts[1] = got[1];
	ch->counts[2] = j->n - got[1];
	/* the spread goes over all records, by their segments */
	j->back = got[0] ? j->n : 0;
	j->idx = d->fc_seg;
	return 0;
}

static int frags_chain_run(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
			   struct xfg_frags_chain *ch, uint8_t *verdicts, void *stream, double *ms)
{
	if (!ctx || !db || !ch || ch->sz < sizeof(*ch) || ch->flags || ((uintptr_t)ch->idx & 3))
		return -EINVAL;
	const uint64_t n = db->count;
	if (n > 0xffffffffull || (n && !verdicts) || (n && descs_bad(db)))
		return -EINVAL;
	if (ms)
		ms[0] = ms[1] = ms[2] = 0;
	if (!n) {
		ch->counts[0] = ch->counts[1] = ch->counts[2] = 0;
		return 0;
	}
	int err = dev_check(ctx, dev);
	if (err)
		return err;
	ch->counts[0] = ch->counts[1] = 0;
	ch->counts[2] = n;
	if (!ch->chain_mask)
		return 0;
	const struct xfg_frags_chain_kargs a = {
		.descs = db->descs, .verdicts = verdicts, .n = (uint32_t)n, .first = db->first,
		.mask = db->mask, .chain_mask = ch->chain_mask,
	};
	struct staged j = {
		.lock = &ctx->dev[dev].frags_lock, .words = XFG_FRAGS_CHAIN_STATE_WORDS(n), .n = n,
		.idx = ch->idx, .verdicts = verdicts, .umem = db->umem,
		.pre = frags_chain_pre, .got = frags_chain_got, .post = xfg_launch_frags_chain_spread,
		.arg = &a, .out = ch,
	};
	return staged_run(ctx, dev, &j, stream, ms);
}

int xfg_classify_descs_frags_chain(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
				   struct xfg_frags_chain *ch, uint8_t *verdicts, void *stream)
{
	return frags_chain_run(ctx, dev, db, ch, verdicts, stream, NULL);
}

int xfg_classify_descs_frags_chain_timed(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
					 struct xfg_frags_chain *ch, uint8_t *verdicts, double ms[3])
{
	return ms ? frags_chain_run(ctx, dev, db, ch, verdicts, NULL, ms) : -EINVAL;
}

/* Many sockets over one UMEM (include/xdpfilter_gpu.h): what both calls check
 * of the sockets; *total their records. */
static int socks_check(const struct xfg_socks *sk, uint64_t *total)
{
	if (!sk || sk->sz < sizeof(*sk) || !sk->socks || !sk->nsocks || sk->nsocks > XFG_SOCKS_MAX)
		return -EINVAL;
	uint64_t n = 0;
	for (uint32_t s = 0; s < sk->nsocks; s++) {
		const struct xfg_sock *k = &sk->socks[s];
		if (!mask_ok(k->rx_mask) || (uint64_t)k->rx_mask + 1 < k->count)
			return -EINVAL;
		if (k->count && (!k->rx_descs || ((uintptr_t)k->rx_descs & 7)))
			return -EINVAL;
		n += k->count;
	}
	if (n > 0xffffffffull)
		return -EINVAL;
	*total = n;
	return 0;
}

/* Staging slot @k, allocated on first use, once its last user -- SOCKS_SLOTS
 * calls ago -- is done (d->lock held, the device current). */
static int socks_slot(struct xfg_dev *d, int k)
{
	int err = 0;
	if (!d->sk_host[k])
		HIPCHK(hipHostMalloc((void **)&d->sk_host[k], SOCKS_SLOT_BYTES, hipHostMallocDefault));
	if (!d->sk_dev[k])
		HIPCHK(hipMalloc((void **)&d->sk_dev[k], SOCKS_SLOT_BYTES));
	if (!d->sk_done[k])
		HIPCHK(hipEventCreateWithFlags(&d->sk_done[k], hipEventDisableTiming));
	HIPCHK(hipEventSynchronize(d->sk_done[k]));
fail:
	return err;
}

/* The socket table of @sk on its way to the device (d->lock held, the device
 * current): into the next staging slot -- waiting for the slot's last user,
 * SOCKS_SLOTS calls ago, only if that is still in flight -- and from there to
 * the slot's device copy on the device's stream.  The caller launches the
 * kernel that reads it and then calls socks_table_done().  With @live
 * (xfg_socks_frags_egress) the table carries, behind the bases, the sockets'
 * live records -- @done[s], or every record where @done is NULL -- and their
 * prefix sums (xfg_layout.h): live[0] and live[1] their device addresses. */
static int socks_table(struct xfg_dev *d, const struct xfg_socks *sk, int *slot,
		       const struct xfg_sock_ent **ents, const uint32_t **base,
		       const uint32_t *done, const uint32_t **live)
{
	int err = 0;
	const int k = (int)d->sk_next;
	if ((err = socks_slot(d, k)))
		return err;
	struct xfg_sock_ent *he = (struct xfg_sock_ent *)d->sk_host[k];
	uint32_t *hb = (uint32_t *)(he + sk->nsocks);
	uint32_t n = 0;
	for (uint32_t s = 0; s < sk->nsocks; s++) {
		const struct xfg_sock *q = &sk->socks[s];
		he[s].rx = (struct xfg_sock_ring){ (uintptr_t)q->rx_descs, q->rx_first, q->rx_mask };
		he[s].tx = (struct xfg_sock_ring){ (uintptr_t)q->tx_descs, q->tx_first, q->tx_mask };
		he[s].fill = (struct xfg_sock_ring){ (uintptr_t)q->fill_addrs, q->fill_first, q->fill_mask };
		hb[s] = n;
		n += q->count;
	}
	hb[sk->nsocks] = n;
	if (live) {
		uint32_t *hd = hb + sk->nsocks + 1, *hp = hd + sk->nsocks;
		n = 0;
		for (uint32_t s = 0; s < sk->nsocks; s++) {
			hd[s] = done ? done[s] : sk->socks[s].count;
			hp[s] = n;
			n += hd[s];
		}
		hp[sk->nsocks] = n;
	}
	HIPCHK(hipMemcpyAsync(d->sk_dev[k], d->sk_host[k],
			      live ? XFG_SOCKS_FRAGS_TABLE_BYTES(sk->nsocks)
				   : XFG_SOCKS_TABLE_BYTES(sk->nsocks),
			      hipMemcpyHostToDevice, d->stream));
	d->sk_next = (uint32_t)(k + 1) % SOCKS_SLOTS;
	*slot = k;
	*ents = (const struct xfg_sock_ent *)d->sk_dev[k];
	*base = (const uint32_t *)(*ents + sk->nsocks);
	if (live) {
		live[0] = *base + sk->nsocks + 1;
		live[1] = live[0] + sk->nsocks;
	}
fail:
	return err;
}

/* ... behind that kernel (or behind the copy alone, if its launch failed:
 * @err, which stands). */
static int socks_table_done(struct xfg_dev *d, int slot, int err)
{
	const int e1 = hip_err(hipEventRecord(d->sk_done[slot], d->stream));
	return err ? err : e1;
}

/* One classify for the sockets' batches, a staged call under socks_lock with
 * nothing read back, so no host synchronisation, and no post-pass: the gather
 * kernel into the caller's flat array or the library's (sized with the stream
 * entered, as scratch_launch()'s launch functions size theirs), then the flat
 * array classified as xfg_classify_descs runs it, into the caller's verdicts. */
static int socks_pre(struct xfg_dev *d, struct staged *j)
{
	const struct xfg_socks *sk = j->arg;
	struct xfg_socks_gather_kargs a = {
		.flat = sk->flat, .n = (uint32_t)j->count, .nsocks = sk->nsocks,
	};
	int err, slot = -1;
	if (!a.flat && (err = scratch(d, &d->sk_flat, &d->sk_flat_bytes, j->count * 16)))
		return err;
	j->descs = a.flat = a.flat ? a.flat : d->sk_flat;
	if ((err = socks_table(d, sk, &slot, &a.ents, &a.base, NULL, NULL)))
		return err;
	err = xfg_launch_socks_gather(&a, (unsigned)d->ncu * 8, d->stream);
	return socks_table_done(d, slot, err);
}

int xfg_classify_socks(xfg_ctx *ctx, int dev, const struct xfg_socks *sk, uint8_t *verdicts,
		       void *stream)
{
	uint64_t total = 0;
	int err;
	if (!ctx)
		return -EINVAL;
	if ((err = socks_check(sk, &total)))
		return err;
	if (((uintptr_t)sk->flat & 15) || (total && (!sk->umem || !verdicts)))
		return -EINVAL;
	if ((err = dev_check(ctx, dev)))
		return err;
	if (!total)
		return 0;
	/* (n = 0: nothing of fr_* is sized) */
	struct staged j = {
		.lock = &ctx->dev[dev].socks_lock, .verdicts = verdicts, .umem = sk->umem,
		.count = total, .pre = socks_pre, .arg = sk,
	};
	return staged_run(ctx, dev, &j, stream, NULL);
}

/* What both egress calls check beyond socks_check(): @flags_ok the flags the
 * call takes. */
static int socks_egress_check(const struct xfg_socks *sk, const struct xfg_socks_egress *e,
			      const uint8_t *verdicts, uint64_t total, uint32_t flags_ok)
{
	if (!e || e->sz < sizeof(*e) || !e->counts || ((uintptr_t)e->counts & 7) ||
	    (e->flags & ~flags_ok) || ((uintptr_t)sk->umem & 7) ||
	    ((e->flags & XFG_EGRESS_SWAP_MACS) && !sk->umem))
		return -EINVAL;
	if (e->fill_addrs && (((uintptr_t)e->fill_addrs & 7) || !mask_ok(e->fill_mask) ||
			      (uint64_t)e->fill_mask + 1 < total))
		return -EINVAL;
	for (uint32_t s = 0; s < sk->nsocks; s++) {
		const struct xfg_sock *k = &sk->socks[s];
		if (k->tx_descs && (((uintptr_t)k->tx_descs & 7) || !mask_ok(k->tx_mask) ||
				    (uint64_t)k->tx_mask + 1 < k->count || (k->count && !verdicts)))
			return -EINVAL;
		if (!e->fill_addrs && k->fill_addrs &&
		    (((uintptr_t)k->fill_addrs & 7) || !mask_ok(k->fill_mask) ||
		     (uint64_t)k->fill_mask + 1 < k->count))
			return -EINVAL;
	}
	return 0;
}

/* Every socket's TX ring and the fill ring(s) in one launch
 * (xfg_socks_egress), and the same over multi-buffer batches
 * (xfg_socks_frags_egress: @frags, with the sockets' @done[] and its prefix
 * sums shipped behind the bases in the same staging slot; a TX record then
 * keeps XDP_PKT_CONTD, so XFG_EGRESS_MULTIBUF is a flag it takes). */
struct socks_egress_job {
	const struct xfg_socks *sk;
	const uint32_t *done;
	int frags;
	struct xfg_socks_frags_egress_kargs a;
};

static int socks_egress_go(struct xfg_dev *d, unsigned grid, void *arg)
{
	struct socks_egress_job *j = arg;
	struct xfg_socks_frags_egress_kargs *a = &j->a;
	const uint32_t *live[2] = { NULL, NULL };
	int slot = -1;
	int err = socks_table(d, j->sk, &slot, &a->ents, &a->base, j->done, j->frags ? live : NULL);
	if (err)
		return err;
	if (j->frags) {
		a->state = d->cstatus;
		a->done = live[0];
		a->dbase = live[1];
		err = xfg_launch_socks_frags_egress(a, grid, d->stream);
	} else {
		/* (the two kernels' argument layouts differ, so field by field: a
		 * field added to struct xfg_socks_kargs is copied here by hand) */
		const struct xfg_socks_kargs b = {
			.umem = a->umem, .ents = a->ents, .base = a->base, .fill = a->fill,
			.verdicts = a->verdicts, .counts = a->counts, .state = d->cstatus,
			.fill_first = a->fill_first, .fill_mask = a->fill_mask,
			.n = a->n, .nsocks = a->nsocks, .swap_macs = a->swap_macs,
		};
		err = xfg_launch_socks_egress(&b, grid, d->stream);
	}
	return socks_table_done(d, slot, err);
}

static int socks_egress(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
			const struct xfg_socks_egress *e, const uint32_t *done,
			const uint8_t *verdicts, void *stream, int frags)
{
	uint64_t total = 0;
	int err;
	if (!ctx)
		return -EINVAL;
	if ((err = socks_check(sk, &total)) ||
	    (err = socks_egress_check(sk, e, verdicts, total,
				      XFG_EGRESS_SWAP_MACS | (frags ? XFG_EGRESS_MULTIBUF : 0))))
		return err;
	for (uint32_t s = 0; done && s < sk->nsocks; s++)
		if (done[s] > sk->socks[s].count)
			return -EINVAL;
	if ((err = dev_check(ctx, dev)))
		return err;
	struct socks_egress_job j = {
		.sk = sk, .done = done, .frags = frags,
		.a = {
			.umem = (e->flags & XFG_EGRESS_SWAP_MACS) ? (uint8_t *)(uintptr_t)sk->umem : NULL,
			.fill = e->fill_addrs, .verdicts = verdicts,
			.counts = (unsigned long long *)e->counts,
			.fill_first = e->fill_first, .fill_mask = e->fill_mask,
			.n = (uint32_t)total, .nsocks = sk->nsocks,
			.swap_macs = !!(e->flags & XFG_EGRESS_SWAP_MACS),
		},
	};
	return scratch_launch(&ctx->dev[dev], stream, total ? NULL : e->counts,
			      (2 * (size_t)sk->nsocks + 2) * 8, XFG_SOCKS_STATE_WORDS(total, sk->nsocks),
			      socks_egress_go, &j);
}

int xfg_socks_egress(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
		     const struct xfg_socks_egress *e, const uint8_t *verdicts, void *stream)
{
	return socks_egress(ctx, dev, sk, e, NULL, verdicts, stream, 0);
}

/* Steered egress (include/xdpfilter_gpu.h): the queues' rings and the avail
 * table reach the device as the socket tables do, through the next staging
 * slot, so the call makes no host synchronisation. */
_Static_assert(XFG_STEER_QUEUES_MAX == XFG_STEER_QUEUES && XFG_STEER_AVAIL_MAX == XFG_STEER_AVAIL &&
	       XFG_QUEUE_NONE == XFG_STEER_NONE, "the kernel's tables");
_Static_assert(XFG_STEER_L4_HASH == XFG_STEER_MODE_HASH && XFG_STEER_L4_SPORT == XFG_STEER_MODE_SPORT &&
	       XFG_STEER_L4_DPORT == XFG_STEER_MODE_DPORT, "the kernel's modes");
_Static_assert(XFG_STEER_TABLE_BYTES(XFG_STEER_QUEUES, XFG_STEER_AVAIL) <= SOCKS_SLOT_BYTES,
	       "a staging slot holds the table");

struct steer_job {
	const struct xfg_steer *s;
	int frags;
	struct xfg_steer_kargs a;
};

static int steer_go(struct xfg_dev *d, unsigned grid, void *arg)
{
	struct steer_job *j = arg;
	const struct xfg_steer *s = j->s;
	struct xfg_steer_kargs *a = &j->a;
	const int k = (int)d->sk_next;
	int err = socks_slot(d, k);
	if (err)
		return err;
	struct xfg_sock_ring *hq = (struct xfg_sock_ring *)d->sk_host[k];
	uint8_t *ha = (uint8_t *)(hq + a->nqueues);
	for (uint32_t q = 0; q < a->nqueues; q++)
		hq[q] = (struct xfg_sock_ring){ (uintptr_t)s->queues[q].tx_descs, s->queues[q].tx_first,
						s->queues[q].tx_mask };
	for (uint32_t i = 0; i < a->navail; i++)
		ha[i] = (uint8_t)(s->avail ? s->avail[i] : i);
	HIPCHK(hipMemcpyAsync(d->sk_dev[k], d->sk_host[k], XFG_STEER_TABLE_BYTES(a->nqueues, a->navail),
			      hipMemcpyHostToDevice, d->stream));
	d->sk_next = (uint32_t)(k + 1) % SOCKS_SLOTS;
	a->queues = (const struct xfg_sock_ring *)d->sk_dev[k];
	a->avail = (const uint8_t *)(a->queues + a->nqueues);
	a->state = d->cstatus;
	err = j->frags ? xfg_launch_steer_frags(a, grid, d->stream) : xfg_launch_steer(a, grid, d->stream);
	return socks_table_done(d, k, err);
fail:
	return err;
}

/* Both steer calls: the single-buffer one, and with @frags the multi-buffer
 * one (the same structure, checks and table; XFG_EGRESS_MULTIBUF is then a flag
 * it takes, and the state has the column of the records that are not live). */
static int steer_egress(xfg_ctx *ctx, int dev, const struct xfg_steer *s, const uint8_t *verdicts,
			void *stream, int frags)
{
	const uint32_t flags_ok = XFG_EGRESS_SWAP_MACS | (frags ? XFG_EGRESS_MULTIBUF : 0);
	int err;
	if (!ctx || !s || s->sz < sizeof(*s) || !s->queues || !s->nqueues ||
	    s->nqueues > XFG_STEER_QUEUES_MAX || s->skip_queue >= s->nqueues ||
	    s->mode > XFG_STEER_L4_DPORT || (s->flags & ~flags_ok) ||
	    s->count > 0xffffffffull || !s->counts)
		return -EINVAL;
	const uint32_t navail = s->avail ? s->navail : s->nqueues;
	if (!navail || navail > XFG_STEER_AVAIL_MAX)
		return -EINVAL;
	if (!mask_ok(s->rx_mask) || (s->fill_addrs && !mask_ok(s->fill_mask)))
		return -EINVAL;
	if (((uintptr_t)s->umem & 7) || ((uintptr_t)s->rx_descs & 7) || ((uintptr_t)s->fill_addrs & 7) ||
	    ((uintptr_t)s->counts & 7))
		return -EINVAL;
	if (s->fill_addrs && (uint64_t)s->fill_mask + 1 < s->count)
		return -EINVAL;
	/* a ring that can be written: one an avail entry or skip_queue names */
	for (uint32_t i = 0; i <= navail; i++) {
		const uint32_t q = i == navail ? s->skip_queue : s->avail ? s->avail[i] : i;
		if (q >= s->nqueues)
			return -EINVAL;
		const struct xfg_steer_queue *k = &s->queues[q];
		if (!k->tx_descs || ((uintptr_t)k->tx_descs & 7) || !mask_ok(k->tx_mask) ||
		    (uint64_t)k->tx_mask + 1 < s->count)
			return -EINVAL;
	}
	if (s->count && (!s->umem || !s->rx_descs || !verdicts))
		return -EINVAL;
	if ((err = dev_check(ctx, dev)))
		return err;
	struct steer_job j = {
		.s = s, .frags = frags,
		.a = {
			.umem = s->umem, .rx = s->rx_descs, .fill = s->fill_addrs, .verdicts = verdicts,
			.queue_of = s->queue_of, .counts = (unsigned long long *)s->counts,
			.rx_first = s->rx_first, .rx_mask = s->rx_mask,
			.fill_first = s->fill_first, .fill_mask = s->fill_mask,
			.n = (uint32_t)s->count, .nqueues = s->nqueues, .navail = navail,
			.mode = s->mode, .skip_queue = s->skip_queue,
			.swap_macs = !!(s->flags & XFG_EGRESS_SWAP_MACS),
		},
	};
	return scratch_launch(&ctx->dev[dev], stream, s->count ? NULL : s->counts,
			      ((size_t)s->nqueues + 2) * 8,
			      frags ? XFG_STEER_FRAGS_STATE_WORDS(s->count, s->nqueues)
				    : XFG_STEER_STATE_WORDS(s->count, s->nqueues),
			      steer_go, &j);
}

int xfg_steer_egress(xfg_ctx *ctx, int dev, const struct xfg_steer *s, const uint8_t *verdicts,
		     void *stream)
{
	return steer_egress(ctx, dev, s, verdicts, stream, 0);
}

int xfg_steer_frags_egress(xfg_ctx *ctx, int dev, const struct xfg_steer *s, const uint8_t *verdicts,
			   void *stream)
{
	return steer_egress(ctx, dev, s, verdicts, stream, 1);
}

/* The forwarding table (include/xdpfilter_gpu.h): xfg_fib.c builds the host
 * copy; on a device context its three arrays are uploaded here, once. */
int xfg_fib_create(xfg_ctx *ctx, int dev, const struct xfg_fib_route *routes, uint64_t nroutes,
		   const struct xfg_fib_nexthop *nexthops, uint32_t nnexthops, xfg_fib **out)
{
	xfg_fib *f = NULL;
	int err;
	if (!ctx || !out || (ctx->ndev && (dev < 0 || dev >= ctx->ndev)))
		return -EINVAL;
	if ((err = xfg_fib_build_host(routes, nroutes, nexthops, nnexthops, &f)))
		return err;
	f->ctx = ctx;
	if (ctx->ndev) {
		const struct { void **d; const void *h; size_t bytes; } up[3] = {
			{ &f->d_t24, f->t24, (size_t)XFG_FIB_T24_ENTRIES * 2 },
			{ &f->d_t8, f->t8, (size_t)(f->ngroups ? f->ngroups : 1) * XFG_FIB_GROUP * 2 },
			{ &f->d_nh, f->nh, (size_t)(f->nnh ? f->nnh : 1) * sizeof(*f->nh) },
		};
		f->dev = dev;
		for (int i = 0; i < 3 && !err; i++) {
			if (!(*up[i].d = xfg_dev_alloc(ctx, dev, up[i].bytes)))
				err = -ENOMEM;
			else
				err = xfg_memcpy_h2d(ctx, dev, *up[i].d, up[i].h, up[i].bytes);
		}
		if (err) {
			xfg_fib_free(f);
			return err;
		}
	}
	*out = f;
	return 0;
}

void xfg_fib_free(xfg_fib *f)
{
	if (!f)
		return;
	if (f->dev >= 0) {
		xfg_dev_free(f->ctx, f->dev, f->d_t24);
		xfg_dev_free(f->ctx, f->dev, f->d_t8);
		xfg_dev_free(f->ctx, f->dev, f->d_nh);
	}
	xfg_fib_free_host(f);
}

/* Forwarded egress (include/xdpfilter_gpu.h): the ports' rings, the stack
 * ring and the ifindex -> queue hash reach the device as the steer call's
 * table does, through the next staging slot. */
_Static_assert(XFG_FWD_PORTS_MAX + 1 == XFG_STEER_QUEUES && XFG_FWD_REASONS == XFG_FWD_NREASONS,
	       "the kernel's tables");
_Static_assert(XFG_FWD_TABLE_BYTES(XFG_STEER_QUEUES) <= SOCKS_SLOT_BYTES, "a staging slot holds the table");
_Static_assert(2 * XFG_FWD_PORTS_MAX <= XFG_FWD_HASH_SLOTS, "a probe meets an empty slot");

struct forward_job {
	const struct xfg_forward *f;
	int frags;
	struct xfg_fwd_kargs a;
};

static int forward_go(struct xfg_dev *d, unsigned grid, void *arg)
{
	struct forward_job *j = arg;
	const struct xfg_forward *f = j->f;
	struct xfg_fwd_kargs *a = &j->a;
	const int k = (int)d->sk_next;
	int err = socks_slot(d, k);
	if (err)
		return err;
	struct xfg_sock_ring *hq = (struct xfg_sock_ring *)d->sk_host[k];
	struct xfg_fwd_slot *hs = (struct xfg_fwd_slot *)(hq + a->nqueues);
	memset(hs, 0, XFG_FWD_HASH_SLOTS * sizeof(*hs));
	for (uint32_t q = 0; q < f->nports; q++) {
		const struct xfg_fwd_port *p = &f->ports[q];
		hq[q] = (struct xfg_sock_ring){ (uintptr_t)p->tx_descs, p->tx_first, p->tx_mask };
		uint32_t s = xfg_fwd_hash(p->ifindex);
		while (hs[s].ifindex)
			s = (s + 1) % XFG_FWD_HASH_SLOTS;
		hs[s] = (struct xfg_fwd_slot){ p->ifindex, q };
	}
	hq[f->nports] = (struct xfg_sock_ring){ (uintptr_t)f->stack.tx_descs, f->stack.tx_first,
						f->stack.tx_mask };
	HIPCHK(hipMemcpyAsync(d->sk_dev[k], d->sk_host[k], XFG_FWD_TABLE_BYTES(a->nqueues),
			      hipMemcpyHostToDevice, d->stream));
	d->sk_next = (uint32_t)(k + 1) % SOCKS_SLOTS;
	a->queues = (const struct xfg_sock_ring *)d->sk_dev[k];
	a->hash = (const struct xfg_fwd_slot *)(a->queues + a->nqueues);
	a->state = d->cstatus;
	err = j->frags ? xfg_launch_forward_frags(a, grid, d->stream) : xfg_launch_forward(a, grid, d->stream);
	return socks_table_done(d, k, err);
fail:
	return err;
}

/* Both forward calls: the single-buffer one, and with @frags the multi-buffer
 * one (the same structure, checks and table; XFG_EGRESS_MULTIBUF is then a flag
 * it takes, and the state has the dead column and the carry column). */
static int forward_egress(xfg_ctx *ctx, int dev, const struct xfg_forward *f, const uint8_t *verdicts,
			  void *stream, int frags)
{
	const uint32_t flags_ok = frags ? XFG_EGRESS_MULTIBUF : 0;
	int err;
	if (!ctx || !f || f->sz < sizeof(*f) || !f->fib || f->fib->ctx != ctx || !f->ports ||
	    !f->nports || f->nports > XFG_FWD_PORTS_MAX || (f->flags & ~flags_ok) ||
	    f->count > 0xffffffffull || !f->counts)
		return -EINVAL;
	if (ctx->ndev && f->fib->dev != dev)
		return -EINVAL;
	if (!mask_ok(f->rx_mask) || (f->fill_addrs && !mask_ok(f->fill_mask)))
		return -EINVAL;
	if (((uintptr_t)f->umem & 7) || ((uintptr_t)f->rx_descs & 7) || ((uintptr_t)f->fill_addrs & 7) ||
	    ((uintptr_t)f->counts & 7))
		return -EINVAL;
	if (f->fill_addrs && (uint64_t)f->fill_mask + 1 < f->count)
		return -EINVAL;
	for (uint32_t q = 0; q <= f->nports; q++) {
		const void *tx = q < f->nports ? f->ports[q].tx_descs : f->stack.tx_descs;
		const uint32_t mask = q < f->nports ? f->ports[q].tx_mask : f->stack.tx_mask;
		if (!tx || ((uintptr_t)tx & 7) || !mask_ok(mask) || (uint64_t)mask + 1 < f->count)
			return -EINVAL;
		if (q == f->nports)
			break;
		if (!f->ports[q].ifindex)
			return -EINVAL;
		for (uint32_t p = 0; p < q; p++)
			if (f->ports[p].ifindex == f->ports[q].ifindex)
				return -EINVAL;
	}
	if (f->count && (!f->umem || !f->rx_descs || !verdicts))
		return -EINVAL;
	if ((err = dev_check(ctx, dev)))
		return err;
	struct forward_job j = {
		.f = f, .frags = frags,
		.a = {
			.umem = f->umem, .rx = f->rx_descs, .t24 = f->fib->d_t24, .t8 = f->fib->d_t8,
			.nh = f->fib->d_nh, .fill = f->fill_addrs, .verdicts = verdicts,
			.queue_of = f->queue_of, .reason_of = f->reason_of,
			.counts = (unsigned long long *)f->counts,
			.rx_first = f->rx_first, .rx_mask = f->rx_mask,
			.fill_first = f->fill_first, .fill_mask = f->fill_mask,
			.n = (uint32_t)f->count, .nqueues = f->nports + 1,
		},
	};
	return scratch_launch(&ctx->dev[dev], stream, f->count ? NULL : f->counts,
			      ((size_t)f->nports + 2 + XFG_FWD_REASONS) * 8,
			      frags ? XFG_FWD_FRAGS_STATE_WORDS(f->count, f->nports + 1)
				    : XFG_STEER_STATE_WORDS(f->count, f->nports + 1),
			      forward_go, &j);
}

int xfg_forward_egress(xfg_ctx *ctx, int dev, const struct xfg_forward *f, const uint8_t *verdicts,
		       void *stream)
{
	return forward_egress(ctx, dev, f, verdicts, stream, 0);
}

int xfg_forward_frags_egress(xfg_ctx *ctx, int dev, const struct xfg_forward *f, const uint8_t *verdicts,
			     void *stream)
{
	return forward_egress(ctx, dev, f, verdicts, stream, 1);
}

/* Multi-buffer batches of many sockets (include/xdpfilter_gpu.h), a staged
 * call: the done pass and the head pass over all the sockets' records, the
 * state words with done[] and the packet count read back through pinned
 * memory, the complete packets' heads classified, and the verdicts spread over
 * all the records, always (a trailing record gets XFG_VERDICT_NONE).  The
 * head, verdict and packet-index scratch is frags_run()'s, so frags_lock keeps
 * a second caller of either off it. */
static int socks_frags_pre(struct xfg_dev *d, struct staged *j)
{
	const struct xfg_socks *sk = j->arg;
	struct xfg_socks_frags_kargs a = {
		.flat = sk->flat, .pkt_of = j->idx, .heads = d->fr_heads, .state = d->cstatus,
		.n = (uint32_t)j->n, .nsocks = sk->nsocks,
	};
	const size_t got_bytes = (XFG_SOCKS_FRAGS_DONE_WORD + XFG_SOCKS_FRAGS_DONE_WORDS(XFG_SOCKS_MAX)) * 8;
	int err, slot = -1;
	if (!d->sf_got &&
	    (err = hip_err(hipHostMalloc((void **)&d->sf_got, got_bytes, hipHostMallocDefault))))
		return err;
	if ((err = socks_table(d, sk, &slot, &a.ents, &a.base, NULL, NULL)))
		return err;
	/* (four workgroups a CU: all of them resident) */
	err = xfg_launch_socks_frags_heads(&a, (unsigned)d->ncu * 4, d->stream);
	return socks_table_done(d, slot, err);
}

static int socks_frags_got(struct xfg_dev *d, struct staged *j)
{
	const struct xfg_socks *sk = j->arg;
	struct xfg_socks_frags *fr = j->out;
	/* state words 1 .. 3 and done[] behind them */
	const uint64_t ngot = XFG_SOCKS_FRAGS_DONE_WORD - 1 + XFG_SOCKS_FRAGS_DONE_WORDS(sk->nsocks);
	const uint32_t *got_done = (const uint32_t *)(d->sf_got + XFG_SOCKS_FRAGS_DONE_WORD - 1);
	uint64_t recs = 0;
	const int err = dev_read(d, d->sf_got, d->cstatus + 1, ngot * 8);
	if (err)
		return err;
	const uint64_t packets = d->sf_got[1];
	for (uint32_t s = 0; s < sk->nsocks; s++) {
		if (got_done[s] > sk->socks[s].count)
			d->sf_got[0] = 1;
		recs += got_done[s];
	}
	/* (word 1: a look-back gave up) */
	if (d->sf_got[0] || packets > recs || (packets != 0) != (recs != 0))
		return -EIO;
	memcpy(fr->done, got_done, (size_t)sk->nsocks * 4);
	fr->counts[0] = j->count = packets;
	fr->counts[1] = recs;
	fr->counts[2] = j->n - recs;
	return 0;
}

int xfg_classify_socks_frags(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
			     struct xfg_socks_frags *fr, uint8_t *verdicts, void *stream)
{
	uint64_t total = 0;
	int err;
	if (!ctx)
		return -EINVAL;
	if ((err = socks_check(sk, &total)))
		return err;
	if (((uintptr_t)sk->flat & 15) || (total && (!sk->umem || !verdicts)))
		return -EINVAL;
	if (!fr || fr->sz < sizeof(*fr) || !fr->done || ((uintptr_t)fr->pkt_of & 3))
		return -EINVAL;
	if ((err = dev_check(ctx, dev)))
		return err;
	memset(fr->done, 0, (size_t)sk->nsocks * 4);
	fr->counts[0] = fr->counts[1] = fr->counts[2] = 0;
	if (!total)
		return 0;
	struct staged j = {
		.lock = &ctx->dev[dev].frags_lock,
		.words = XFG_SOCKS_FRAGS_STATE_WORDS(total, sk->nsocks), .n = total, .idx = fr->pkt_of,
		.verdicts = verdicts, .umem = sk->umem, .back = total,
		.pre = socks_frags_pre, .got = socks_frags_got, .post = xfg_launch_socks_frags_spread,
		.arg = sk, .out = fr,
	};
	return staged_run(ctx, dev, &j, stream, NULL);
}

/* ... and their egress */
int xfg_socks_frags_egress(xfg_ctx *ctx, int dev, const struct xfg_socks *sk,
			   const struct xfg_socks_egress *e, const uint32_t *done,
			   const uint8_t *verdicts, void *stream)
{
	return socks_egress(ctx, dev, sk, e, done, verdicts, stream, 1);
}

/* Capture by verdict (include/xdpfilter_gpu.h): what every capture call
 * checks of @c, the device and its batch of @count frames in @base ... */
static int capture_check(xfg_ctx *ctx, int dev, const struct xfg_capture *c, const void *verdicts,
			 const void *base, uint64_t count)
{
	if (!c || c->sz < sizeof(*c) || !c->counts || ((uintptr_t)c->counts & 7) ||
	    ((uintptr_t)c->ts_ns & 7) || ((uintptr_t)c->out & 15) || (!c->out && c->out_bytes) ||
	    (!verdicts && count) || count > 0xffffffffull)
		return -EINVAL;
	int err = dev_check(ctx, dev);
	if (err)
		return err;
	return count && !base ? -EINVAL : 0;
}

/* ... and of a descriptor batch */
static int capture_descs_check(xfg_ctx *ctx, const struct xfg_desc_batch *db)
{
	if (!ctx || !db || !mask_ok(db->mask))
		return -EINVAL;
	if (db->count && !db->descs)
		return -EINVAL;
	if (((uintptr_t)db->descs & 7) || ((uintptr_t)db->umem & 15))
		return -EINVAL;
	return 0;
}

static int capture_go(struct xfg_dev *d, unsigned grid, void *arg)
{
	struct xfg_capture_kargs *a = arg;
	a->state = d->cstatus;
	return xfg_launch_capture(a, grid, d->stream);
}

/* Both single-record entry points fill the kernel's arguments but for the
 * launch's own and come here; nothing selected counts as an empty batch. */
static int capture_launch(xfg_ctx *ctx, int dev, struct xfg_capture_kargs *a, uint64_t count,
			  const struct xfg_capture *c, void *stream)
{
	int err = capture_check(ctx, dev, c, a->verdicts, a->base, count);
	if (err)
		return err;
	a->ts_ns = c->ts_ns;
	a->ts0 = c->ts0;
	a->out = c->out;
	a->out_bytes = c->out_bytes;
	a->counts = (unsigned long long *)c->counts;
	a->n = (uint32_t)count;
	a->action_mask = c->action_mask;
	a->snaplen = c->snaplen;
	return scratch_launch(&ctx->dev[dev], stream, count && c->action_mask ? NULL : c->counts, 24,
			      XFG_CAPTURE_STATE_WORDS(count), capture_go, a);
}

int xfg_capture(xfg_ctx *ctx, int dev, const struct xfg_batch *b, const uint8_t *verdicts,
		const struct xfg_capture *c, void *stream)
{
	if (!ctx || !b)
		return -EINVAL;
	if (b->count && !b->lens)
		return -EINVAL;
	if (!b->offsets && b->count && (b->stride == 0 || (b->stride & 15)))
		return -EINVAL;
	if (((uintptr_t)b->data & 15) || ((uintptr_t)b->offsets & 7) ||
	    ((uintptr_t)b->lens & (b->lens_u16 ? 1 : 3)))
		return -EINVAL;
	struct xfg_capture_kargs a = {
		.base = b->data, .offsets = b->offsets, .lens = b->lens, .verdicts = verdicts,
		.stride = b->stride, .form = b->lens_u16 ? XFG_CAPTURE_F_LENS_U16 : 0,
	};
	return capture_launch(ctx, dev, &a, b->count, c, stream);
}

int xfg_capture_descs(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
		      const uint8_t *verdicts, const struct xfg_capture *c, void *stream)
{
	int err = capture_descs_check(ctx, db);
	if (err)
		return err;
	struct xfg_capture_kargs a = {
		.base = db->umem, .descs = db->descs, .verdicts = verdicts,
		.first = db->first, .mask = db->mask, .form = XFG_CAPTURE_F_DESCS,
	};
	return capture_launch(ctx, dev, &a, db->count, c, stream);
}

/* Capture of multi-buffer packets, one block a packet (include/
 * xdpfilter_gpu.h): two kernels, two sets of status words in one request, and
 * the per-record scratch of the scan. */
static int capture_frags_go(struct xfg_dev *d, unsigned grid, void *arg)
{
	struct xfg_capture_frags_kargs *a = arg;
	int err;
	if ((err = scratch(d, (void **)&d->cf_off, &d->cf_off_bytes, (uint64_t)a->n * 4)) ||
	    (err = scratch(d, (void **)&d->cf_tot, &d->cf_tot_bytes, (uint64_t)a->n * 8)))
		return err;
	a->state = d->cstatus;
	a->off = d->cf_off;
	a->tot = d->cf_tot;
	return xfg_launch_capture_frags(a, grid, d->stream);
}

int xfg_capture_descs_frags(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *db,
			    const uint8_t *verdicts, const struct xfg_capture *c, uint32_t flags,
			    void *stream)
{
	int err = capture_descs_check(ctx, db);
	if (err || (flags & ~XFG_CAPTURE_HEAD_ONLY))
		return -EINVAL;
	if ((err = capture_check(ctx, dev, c, verdicts, db->umem, db->count)))
		return err;
	struct xfg_capture_frags_kargs a = {
		.umem = db->umem, .descs = db->descs, .verdicts = verdicts,
		.ts_ns = c->ts_ns, .ts0 = c->ts0, .out = c->out, .out_bytes = c->out_bytes,
		.counts = (unsigned long long *)c->counts,
		.n = (uint32_t)db->count, .first = db->first, .mask = db->mask,
		.action_mask = c->action_mask, .snaplen = c->snaplen,
		.head_only = !!(flags & XFG_CAPTURE_HEAD_ONLY),
	};
	return scratch_launch(&ctx->dev[dev], stream, db->count && c->action_mask ? NULL : c->counts,
			      24, XFG_CAPTURE_FRAGS_STATE_WORDS(db->count), capture_frags_go, &a);
}

/* Achievable streaming-read rate of the device (bench.py roofline leg). */
int xfg_stream_read_timed(xfg_ctx *ctx, int dev, const void *src, uint64_t bytes, int iters,
			  double *avg_ms)
{
	int err = 0;
	float ms = 0;
	if (!ctx || dev < 0 || dev >= ctx->ndev || !avg_ms || iters < 1)
		return -EINVAL;
	struct xfg_dev *d = &ctx->dev[dev];
	unsigned grid = (unsigned)d->ncu * 8;
	HIPCHK(hipSetDevice(d->ordinal));
	HIPCHK(hipEventRecord(d->ev0, d->stream));
	for (int i = 0; i < iters; i++)
		if ((err = xfg_launch_stream_read(src, bytes, d->sink, grid, d->stream)))
			goto fail;
	HIPCHK(hipEventRecord(d->ev1, d->stream));
	HIPCHK(hipEventSynchronize(d->ev1));
	HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
	*avg_ms = ms / iters;
	return 0;
fail:
	return err;
}

/* Host-resident batches (xfg_classify_host, xfg_classify_xsk_host).
 *
 * Only header windows cross PCIe: each packet's first HOST_WIN bytes go to
 * a pinned staging slot (gathered by the device's thread pool) with its
 * true length, H2D, and the general kernel classifies them in header-window
 * mode (kargs.hwin).  A packet whose program would read past its window
 * (long IPv6 extension chains and the like) is not classified or counted
 * there: the kernel lists it, and the host sends its whole frame through
 * the ordinary device path afterwards -- the verdicts, counters and stats
 * are exactly those of a whole-frame run.  A fixed-stride batch whose
 * stride is at most HOST_WIN is staged slot for slot instead (one memcpy
 * per slice; nothing can fall back).  HOST_SLOTS staging slots of HOST_CH
 * packets rotate (gather / H2D / kernel / D2H, each slot on its own
 * stream); their size is fixed (HOST_CH x HOST_WIN bytes each), whatever
 * the frames' lengths.
 * One lock per device: the devices' host paths run concurrently. */
#define HOST_CH (1u << 18)     /* packets per staging slot */
#define HOST_WIN 128u          /* header window (bytes) */
#define FB_BYTES (64u << 20)   /* whole-frame fallback staging */
#define FB_PKTS (1u << 16)     /* ... and its packets per pass */

/* where packet i of a host batch lies */
struct hsrc {
	const uint8_t *data;       /* batch data, or the UMEM */
	const uint64_t *offsets;
	uint32_t stride;
	const void *lens;
	int lens_u16;
	const uint64_t *descs;     /* AF_XDP RX ring (xdp_desc records), or NULL */
	uint32_t first, mask;
	uint64_t span;             /* descs: the bytes from the UMEM's start the
				    * kernels' 16-byte loads may touch */
};

static inline const uint8_t *hsrc_ptr(const struct hsrc *s, uint64_t i)
{
	if (s->descs) {
		/* xsk_umem__add_offset_to_addr(): unaligned-chunk offset in
		 * bits 48..63 (headers/xdp/xsk.h:173-186) */
		const uint64_t a = s->descs[2ull * ((s->first + (uint32_t)i) & s->mask)];
		return s->data + (a & ((1ull << 48) - 1)) + (a >> 48);
	}
	return s->data + (s->offsets ? s->offsets[i] : i * (uint64_t)s->stride);
}

static inline uint32_t hsrc_len(const struct hsrc *s, uint64_t i)
{
	if (s->descs)   /* xdp_desc.len: the low half of the record's second word */
		return (uint32_t)s->descs[2ull * ((s->first + (uint32_t)i) & s->mask) + 1];
	const uint32_t l = s->lens_u16 ? ((const uint16_t *)s->lens)[i] : ((const uint32_t *)s->lens)[i];
	/* a fixed-stride frame lies in its slot: a longer length is capped at the
	 * slot, as the device path caps it (the gather, the kernel and the
	 * whole-frame fallback then all see the same length, and no copy reads
	 * past the slot) */
	return (!s->offsets && s->stride && l > s->stride) ? s->stride : l;
}

struct gather_job {
	const struct hsrc *src;
	uint64_t first, m;         /* packets [first, first + m) */
	uint8_t *dst;
	uint32_t *dl;
	uint32_t stride;           /* staging stride: HOST_WIN, or the batch's */
	int whole;                 /* 1 whole slots copied (stride <= HOST_WIN, no
				    * offsets), 2 whole slots left where they lie
				    * (registered memory: lengths only), 3 frames
				    * left where they lie in a registered UMEM
				    * (offsets into dst, lengths), 4 the caller's
				    * lengths as they are (dl: u16 or u32; the
				    * kernels cap them at the stride), 0 windows */
};

static void gather_slice(void *arg, int t, int nt)
{
	const struct gather_job *j = arg;
	const uint64_t per = (j->m + nt - 1) / nt;
	const uint64_t s0 = t * per, s1 = s0 + per < j->m ? s0 + per : j->m;
	if (s0 >= s1)
		return;
	if (j->whole == 4) {
		const size_t ls = j->src->lens_u16 ? 2 : 4;
		memcpy((uint8_t *)j->dl + s0 * ls, (const uint8_t *)j->src->lens + (j->first + s0) * ls,
		       (s1 - s0) * ls);
		return;
	}
	if (j->whole == 1)
		memcpy(j->dst + s0 * j->stride, j->src->data + (j->first + s0) * j->stride,
		       (s1 - s0) * j->stride);
	for (uint64_t i = s0; i < s1; i++) {
		const uint32_t l = hsrc_len(j->src, j->first + i);
		if (j->whole == 3)
			((uint64_t *)j->dst)[i] = (uint64_t)(hsrc_ptr(j->src, j->first + i) - j->src->data);
		else if (!j->whole)
			memcpy(j->dst + i * HOST_WIN, hsrc_ptr(j->src, j->first + i),
			       l < HOST_WIN ? l : HOST_WIN);
		j->dl[i] = l;
	}
}

static int host_staging(struct xfg_dev *d)
{
	int err = 0;
	if (!d->pool && !(d->pool = hpool_start()))
		return -ENOMEM;
	if (d->hs_st[0])
		return 0;
	for (int k = 0; k < HOST_SLOTS; k++) {
		HIPCHK(hipStreamCreateWithFlags(&d->hs_st[k], hipStreamNonBlocking));
		HIPCHK(hipEventCreate(&d->hs_done[k]));
		HIPCHK(hipHostMalloc((void **)&d->hs_hbuf[k], (size_t)HOST_CH * HOST_WIN,
				     hipHostMallocDefault));
		HIPCHK(hipHostMalloc((void **)&d->hs_hl[k], HOST_CH * 4, hipHostMallocDefault));
		HIPCHK(hipHostMalloc((void **)&d->hs_hfbc[k], 4, hipHostMallocDefault));
		HIPCHK(hipMalloc((void **)&d->hs_dbuf[k], (size_t)HOST_CH * HOST_WIN));
		HIPCHK(hipMalloc((void **)&d->hs_dl[k], HOST_CH * 4));
		HIPCHK(hipMalloc((void **)&d->hs_dv[k], HOST_CH));
		HIPCHK(hipMalloc((void **)&d->hs_fb[k], HOST_CH * 4));
		HIPCHK(hipMalloc((void **)&d->hs_fbc[k], 4));
	}
	return 0;
fail:
	for (int k = 0; k < HOST_SLOTS; k++) {   /* all or nothing: a later call starts over */
		if (d->hs_st[k])
			hipStreamDestroy(d->hs_st[k]);
		if (d->hs_done[k])
			hipEventDestroy(d->hs_done[k]);
		hipHostFree(d->hs_hbuf[k]);
		hipHostFree(d->hs_hl[k]);
		hipHostFree(d->hs_hfbc[k]);
		hipFree(d->hs_dbuf[k]);
		hipFree(d->hs_dl[k]);
		hipFree(d->hs_dv[k]);
		hipFree(d->hs_fb[k]);
		hipFree(d->hs_fbc[k]);
		d->hs_st[k] = NULL;
		d->hs_done[k] = NULL;
		d->hs_hbuf[k] = d->hs_dbuf[k] = d->hs_dv[k] = NULL;
		d->hs_hl[k] = d->hs_dl[k] = d->hs_fb[k] = d->hs_fbc[k] = d->hs_hfbc[k] = NULL;
	}
	return err;
}

static int fb_staging(struct xfg_dev *d)
{
	int err = 0;
	if (d->fb_h)
		return 0;
	HIPCHK(hipHostMalloc((void **)&d->fb_ho, FB_PKTS * 8, hipHostMallocDefault));
	HIPCHK(hipHostMalloc((void **)&d->fb_hl, FB_PKTS * 4, hipHostMallocDefault));
	HIPCHK(hipHostMalloc((void **)&d->fb_idx, (size_t)HOST_CH * 4, hipHostMallocDefault));
	HIPCHK(hipMalloc((void **)&d->fb_d, FB_BYTES + 64));
	HIPCHK(hipMalloc((void **)&d->fb_do, FB_PKTS * 8));
	HIPCHK(hipMalloc((void **)&d->fb_dl, FB_PKTS * 4));
	HIPCHK(hipMalloc((void **)&d->fb_dv, FB_PKTS));
	HIPCHK(hipHostMalloc((void **)&d->fb_h, FB_BYTES + 64, hipHostMallocDefault));
	return 0;
fail:
	hipHostFree(d->fb_ho);
	hipHostFree(d->fb_hl);
	hipHostFree(d->fb_idx);
	hipFree(d->fb_d);
	hipFree(d->fb_do);
	hipFree(d->fb_dl);
	hipFree(d->fb_dv);
	d->fb_ho = NULL;
	d->fb_hl = d->fb_idx = d->fb_dl = NULL;
	d->fb_d = d->fb_dv = NULL;
	d->fb_do = NULL;
	return err;
}

/* Classify a device-resident sub-batch on stream st (kernels on the device
 * stream, ordered after st's uploads; st after the kernels). */
static int host_launch(xfg_ctx *ctx, struct xfg_dev *d, const struct xfg_batch *sub,
		       uint8_t *dv, int hwin, uint32_t *fb, uint32_t *fbc, hipStream_t st)
{
	struct launch l;
	int err = snapshot(ctx, d, sub, NULL, dv, hwin, &l);
	if (err)
		return err;
	if (hwin) {   /* header windows (the general kernel): listing what leaves them */
		l.a.fb = fb;
		l.a.fb_cnt = fbc;
		l.a.fb_cap = HOST_CH;
	}
	return launch_batch(ctx, d, &l, st, 1);
}

/* The packets of the chunk at `c` whose programs left their windows (count
 * in *d->hs_hfbc[k], list in d->hs_fb[k]): their whole frames through the
 * ordinary path, FB_BYTES / FB_PKTS at a time; verdicts scattered back. */
static int host_fallback(xfg_ctx *ctx, struct xfg_dev *d, const struct hsrc *src, uint64_t c,
			 int k, uint8_t *verdicts)
{
	int err = 0;
	const uint32_t nf = *d->hs_hfbc[k];
	if (!nf)
		return 0;
	if (nf > HOST_CH)
		return -EIO;
	if ((err = fb_staging(d)))
		return err;
	HIPCHK(hipMemcpyAsync(d->fb_idx, d->hs_fb[k], (size_t)nf * 4, hipMemcpyDeviceToHost,
			      d->hs_st[k]));
	HIPCHK(hipStreamSynchronize(d->hs_st[k]));
	for (uint32_t j0 = 0; j0 < nf;) {
		uint64_t pos = 0;
		uint32_t m = 0;
		while (j0 + m < nf && m < FB_PKTS) {
			const uint64_t gi = c + d->fb_idx[j0 + m];
			const uint32_t l = hsrc_len(src, gi);
			if (l > FB_BYTES)
				return -E2BIG;
			if (pos + l > FB_BYTES)
				break;
			memcpy(d->fb_h + pos, hsrc_ptr(src, gi), l);
			d->fb_ho[m] = pos;
			d->fb_hl[m] = l;
			pos = (pos + l + 15) & ~15ull;   /* 16-byte aligned starts */
			m++;
		}
		HIPCHK(hipMemcpyAsync(d->fb_d, d->fb_h, pos, hipMemcpyHostToDevice, d->hs_st[k]));
		HIPCHK(hipMemcpyAsync(d->fb_do, d->fb_ho, (size_t)m * 8, hipMemcpyHostToDevice,
				      d->hs_st[k]));
		HIPCHK(hipMemcpyAsync(d->fb_dl, d->fb_hl, (size_t)m * 4, hipMemcpyHostToDevice,
				      d->hs_st[k]));
		struct xfg_batch sub = { d->fb_d, d->fb_do, d->fb_dl, m, 0, 0 };
		if ((err = host_launch(ctx, d, &sub, d->fb_dv, 0, NULL, NULL, d->hs_st[k])))
			return err;
		/* (the pinned frame buffer doubles as the verdicts' landing place) */
		HIPCHK(hipMemcpyAsync(d->fb_h, d->fb_dv, m, hipMemcpyDeviceToHost, d->hs_st[k]));
		HIPCHK(hipStreamSynchronize(d->hs_st[k]));
		for (uint32_t q = 0; q < m; q++)
			verdicts[c + d->fb_idx[j0 + q]] = d->fb_h[q];
		j0 += m;
	}
	*d->hs_hfbc[k] = 0;
	return 0;
fail:
	return err;
}

/* ---- registered host buffers: DMA straight from the caller's memory */
int xfg_host_register(xfg_ctx *ctx, void *p, size_t bytes)
{
	int err = 0;
	if (!ctx || !p || !bytes)
		return -EINVAL;
	pthread_mutex_lock(&ctx->reg_lock);
	for (int i = 0; i < ctx->nreg; i++) {
		const uint8_t *a = ctx->reg[i].p, *b = (const uint8_t *)p;
		if (b < a + ctx->reg[i].bytes && a < b + bytes) {
			err = -EEXIST;   /* overlaps a registered buffer */
			goto out;
		}
	}
	if (ctx->nreg == XFG_HOST_REG_MAX) {
		err = -ENOSPC;
		goto out;
	}
	/* mapped as well: whole slots are read by the kernels where they lie
	 * (host_run's zero-copy path) */
	if ((err = hip_err(hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped))))
		goto out;
	ctx->reg[ctx->nreg].p = p;
	ctx->reg[ctx->nreg].bytes = bytes;
	ctx->nreg++;
out:
	pthread_mutex_unlock(&ctx->reg_lock);
	return err;
}

int xfg_host_unregister(xfg_ctx *ctx, void *p)
{
	int err = -ENOENT;
	if (!ctx || !p)
		return -EINVAL;
	/* (no host-path call may be using it: the caller's contract, as for
	 * freeing any buffer it passed) */
	pthread_mutex_lock(&ctx->reg_lock);
	for (int i = 0; i < ctx->nreg; i++) {
		if (ctx->reg[i].p != p)
			continue;
		err = hip_err(hipHostUnregister(p));
		ctx->reg[i] = ctx->reg[--ctx->nreg];
		break;
	}
	pthread_mutex_unlock(&ctx->reg_lock);
	return err;
}

/* Whether [p, p + bytes) lies inside one registered buffer (*base: that
 * buffer's start). */
static int host_registered(xfg_ctx *ctx, const void *p, uint64_t bytes, const uint8_t **base)
{
	int r = 0;
	pthread_mutex_lock(&ctx->reg_lock);
	for (int i = 0; i < ctx->nreg && !r; i++)
		if ((r = (const uint8_t *)p >= ctx->reg[i].p &&
			 (const uint8_t *)p + bytes <= ctx->reg[i].p + ctx->reg[i].bytes) && base)
			*base = ctx->reg[i].p;
	pthread_mutex_unlock(&ctx->reg_lock);
	return r;
}

/* Zero copy: the batch's frames read by the kernels through the registered
 * buffer's device mapping; per chunk the pool copies the lengths (for
 * AF_XDP: gathers the frames' UMEM offsets and lengths) into the slot's
 * pinned buffer, one H2D copy takes them to the slot's device buffer, the
 * kernels run, the verdicts come back.  Chunks of 2^22 packets (AF_XDP:
 * 2^21), far larger than the staged path's: the kernels' reads cross PCIe
 * at its latency, and a short launch ramps up and drains for a larger share
 * of its time (C3, u32 lengths: 2^18-packet chunks 430 Mpps, 2^21 630, one
 * launch from device-resident lengths 790). */
#define ZC_CH (1u << 21)   /* AF_XDP (13 bytes a packet); fixed stride: twice (5 bytes) */
#ifndef HYB_ZC_CH   /* host_run_hyb: packets of a round's zero-copy chunk, ... */
#define HYB_ZC_CH (1ull << 20)
#endif
#ifndef HYB_ST_N    /* ... and its staged chunks of HOST_CH (0: no hybrid) */
/* (off: on C5 from a registered buffer, 2^23 frames of 1514 B, zero copy
 * alone ran 270 Mpps and every hybrid setting tried 175-220 -- the staged
 * gather's reads of the same host memory slow the kernels' PCIe reads more
 * than its chunks add, profiles/r06_s6_hyb_c5.log; the diagnostics build
 * still takes XFG_HYB_ZLOG2 / XFG_HYB_ST) */
#define HYB_ST_N 0u
#endif
_Static_assert((size_t)ZC_CH * 13 + 256 <= (size_t)HOST_CH * HOST_WIN, "slot buffers hold a chunk");
_Static_assert((size_t)ZC_CH * 2 * 5 + 256 <= (size_t)HOST_CH * HOST_WIN, "slot buffers hold a chunk");

static int host_run_zc(xfg_ctx *ctx, struct xfg_dev *d, const struct hsrc *src, uint64_t n,
		       const uint8_t *rbase, uint8_t *verdicts)
{
	int err = 0;
	void *dp = NULL;
	HIPCHK(hipHostGetDevicePointer(&dp, (void *)rbase, 0));
	const uint8_t *zdev = (const uint8_t *)dp + (src->data - rbase);   /* the batch, device side */
	/* (chunks growing from 2^17, so that the first kernel starts after a
	 * short copy, measured slower: 607 Mpps against 670 for C3) */
	uint64_t ch = src->descs ? ZC_CH : 2 * ZC_CH;
#ifdef XFG_DIAG
	const char *zl = getenv("XFG_ZC_LOG2");   /* chunk size (log2, at most the default) */
	if (zl && atoi(zl) >= 12 && (1ull << atoi(zl)) <= ch)
		ch = 1ull << atoi(zl);
#endif
	/* fixed-stride lengths go as the caller holds them (u16 or u32) */
	const size_t ls = src->descs ? 4 : src->lens_u16 ? 2 : 4;
	for (uint64_t c = 0, k = 0; c < n; c += ch, k = (k + 1) % HOST_SLOTS) {
		const uint64_t m = n - c < ch ? n - c : ch;
		/* slot layout (pinned and device alike): [offsets u64 x m] lens x m;
		 * verdicts after them, device side */
		const size_t ob = src->descs ? m * 8 : 0, lb = ob + m * ls, vb = (lb + 255) & ~(size_t)255;
		HIPCHK(hipEventSynchronize(d->hs_done[k]));   /* slot k free again */
		struct gather_job job = { src, c, m, d->hs_hbuf[k], (uint32_t *)(d->hs_hbuf[k] + ob),
					  HOST_WIN, src->descs ? 3 : 4 };
		hpool_run(d->pool, gather_slice, &job);
		HIPCHK(hipMemcpyAsync(d->hs_dbuf[k], d->hs_hbuf[k], lb, hipMemcpyHostToDevice, d->hs_st[k]));
		struct xfg_batch sub = { zdev + (src->descs ? 0 : c * src->stride),
					 src->descs ? (const uint64_t *)d->hs_dbuf[k] : NULL,
					 d->hs_dbuf[k] + ob, m, src->descs ? 0 : src->stride, ls == 2 };
		if ((err = host_launch(ctx, d, &sub, d->hs_dbuf[k] + vb, 0, NULL, NULL, d->hs_st[k])))
			goto fail;
		HIPCHK(hipMemcpyAsync(verdicts + c, d->hs_dbuf[k] + vb, m, hipMemcpyDeviceToHost,
				      d->hs_st[k]));
		HIPCHK(hipEventRecord(d->hs_done[k], d->hs_st[k]));
	}
	for (int k = 0; k < HOST_SLOTS; k++)
		HIPCHK(hipStreamSynchronize(d->hs_st[k]));
fail:
	return err;
}

/* Registered large slots (C5's 1514-byte frames at a 1536-byte stride): the
 * zero-copy kernels are bound by the rate of PCIe read requests (one 64-byte
 * window a frame, ~0.3 Gpps) and the staged path by the pool's gather (~0.13
 * Gpps), different resources -- so each round takes one zero-copy chunk of
 * zc_ch packets (its kernel reading mapped host memory while the pool works)
 * and then st_n staged chunks of header windows (gathered meanwhile, their
 * kernels queued behind it): slots 0-1 for the zero-copy chunks, 2-3 for the
 * staged ones.  Verdicts, counters and stats are those of either path: the
 * same kernels over the same frames, the staged windows' leavers walked
 * whole (host_fallback). */
static int host_run_hyb(xfg_ctx *ctx, struct xfg_dev *d, const struct hsrc *src, uint64_t n,
			const uint8_t *rbase, uint8_t *verdicts, uint64_t zc_ch, uint32_t st_n)
{
	int err = 0;
	void *dp = NULL;
	HIPCHK(hipHostGetDevicePointer(&dp, (void *)rbase, 0));
	const uint8_t *zdev = (const uint8_t *)dp + (src->data - rbase);
	const size_t ls = src->lens_u16 ? 2 : 4;
	uint64_t pend[HOST_SLOTS];
	for (int k = 0; k < HOST_SLOTS; k++)
		pend[k] = UINT64_MAX;
	uint32_t zk = 0, sk = 0;
	for (uint64_t c = 0; c < n;) {
		/* the zero-copy chunk: the pool copies its lengths, the kernel
		 * reads the frames where they lie */
		{
			const int k = (int)(zk++ & 1);
			const uint64_t m = n - c < zc_ch ? n - c : zc_ch;
			const size_t lb = m * ls, vb = (lb + 255) & ~(size_t)255;
			HIPCHK(hipEventSynchronize(d->hs_done[k]));
			struct gather_job job = { src, c, m, d->hs_hbuf[k], (uint32_t *)d->hs_hbuf[k], HOST_WIN, 4 };
			hpool_run(d->pool, gather_slice, &job);
			HIPCHK(hipMemcpyAsync(d->hs_dbuf[k], d->hs_hbuf[k], lb, hipMemcpyHostToDevice, d->hs_st[k]));
			struct xfg_batch sub = { zdev + c * src->stride, NULL, d->hs_dbuf[k], m, src->stride, ls == 2 };
			if ((err = host_launch(ctx, d, &sub, d->hs_dbuf[k] + vb, 0, NULL, NULL, d->hs_st[k])))
				goto fail;
			HIPCHK(hipMemcpyAsync(verdicts + c, d->hs_dbuf[k] + vb, m, hipMemcpyDeviceToHost,
					      d->hs_st[k]));
			HIPCHK(hipEventRecord(d->hs_done[k], d->hs_st[k]));
			c += m;
		}
		/* the staged chunks: 128-byte header windows gathered by the pool
		 * while the zero-copy kernel runs */
		for (uint32_t j = 0; j < st_n && c < n; j++) {
			const int k = 2 + (int)(sk++ & 1);
			const uint64_t m = n - c < HOST_CH ? n - c : HOST_CH;
			HIPCHK(hipEventSynchronize(d->hs_done[k]));
			if (pend[k] != UINT64_MAX && (err = host_fallback(ctx, d, src, pend[k], k, verdicts)))
				goto fail;
			struct gather_job job = { src, c, m, d->hs_hbuf[k], d->hs_hl[k], HOST_WIN, 0 };
			hpool_run(d->pool, gather_slice, &job);
			HIPCHK(hipMemcpyAsync(d->hs_dbuf[k], d->hs_hbuf[k], m * HOST_WIN, hipMemcpyHostToDevice,
					      d->hs_st[k]));
			HIPCHK(hipMemcpyAsync(d->hs_dl[k], d->hs_hl[k], m * 4, hipMemcpyHostToDevice, d->hs_st[k]));
			HIPCHK(hipMemsetAsync(d->hs_fbc[k], 0, 4, d->hs_st[k]));
			struct xfg_batch sub = { d->hs_dbuf[k], NULL, d->hs_dl[k], m, HOST_WIN, 0 };
			if ((err = host_launch(ctx, d, &sub, d->hs_dv[k], 1, d->hs_fb[k], d->hs_fbc[k],
					       d->hs_st[k])))
				goto fail;
			HIPCHK(hipMemcpyAsync(verdicts + c, d->hs_dv[k], m, hipMemcpyDeviceToHost, d->hs_st[k]));
			HIPCHK(hipMemcpyAsync(d->hs_hfbc[k], d->hs_fbc[k], 4, hipMemcpyDeviceToHost, d->hs_st[k]));
			HIPCHK(hipEventRecord(d->hs_done[k], d->hs_st[k]));
			pend[k] = c;
			c += m;
		}
	}
	for (int k = 0; k < HOST_SLOTS; k++) {
		HIPCHK(hipStreamSynchronize(d->hs_st[k]));
		if (pend[k] != UINT64_MAX && (err = host_fallback(ctx, d, src, pend[k], k, verdicts)))
			goto fail;
	}
fail:
	return err;
}

static int host_run(xfg_ctx *ctx, int dev, const struct hsrc *src, uint64_t n, uint8_t *verdicts)
{
	int err = 0;
	struct xfg_dev *d = &ctx->dev[dev];
	/* whole slots: a fixed stride within the window (16-byte aligned, or
	 * the kernel's 16-byte loads would straddle slots) */
	const int whole = !src->descs && !src->offsets && src->stride && src->stride <= HOST_WIN &&
			  !(src->stride & 15);
	const uint32_t stride = whole ? src->stride : HOST_WIN;
	/* fixed-stride slots (16-byte aligned) in a registered buffer: read by
	 * the kernels where they lie, through the buffer's device mapping (zero
	 * copy: the kernel's loads cross PCIe, the window and whatever a
	 * program walks past it, nothing else; whole frames in view, so no
	 * fallback) -- the pool gathers the lengths only.  Measured on MI355X
	 * against one DMA of the whole slots per chunk (C3, 64-byte frames,
	 * bench.py's host_path): 41-46 GB/s of frames against 34-36 on this
	 * round's boxes (profiles/archive/r05_s16..s19, s36, s47).  The
	 * slots must start 16-byte aligned, as the device path's batches do
	 * (check_batch): an unaligned registered batch takes the staged path. */
	const uint8_t *rbase = NULL;
	int zc = (!src->descs && !src->offsets && src->stride && !(src->stride & 15) &&
		  !((uintptr_t)src->data & 15) &&
		  host_registered(ctx, src->data, n * (uint64_t)src->stride, &rbase)) ||
		 /* AF_XDP frames in a registered UMEM: the descriptors' offsets
		  * and lengths gathered, the frames read in place */
		 (src->descs && host_registered(ctx, src->data, src->span, &rbase));
#ifdef XFG_DIAG
	const char *zs = getenv("XFG_HOST_ZC");   /* "off": round 4's DMA paths */
	if (zs && !strcmp(zs, "off"))
		zc = 0;
#endif
	/* whole slots in a registered buffer: copied by DMA where they lie */
	const int direct = !zc && whole && host_registered(ctx, src->data, n * (uint64_t)stride, NULL);
	/* windows of larger slots in a registered buffer: one strided DMA per
	 * chunk (rows of HOST_WIN bytes at the batch's stride; a window never
	 * leaves its slot) instead of the pool's gather -- the pool then
	 * gathers the lengths only */
	const int direct2d = !zc && !whole && !src->descs && !src->offsets && src->stride > HOST_WIN &&
			     !(src->stride & 15) &&
			     host_registered(ctx, src->data, n * (uint64_t)src->stride, NULL);
	uint64_t pend[HOST_SLOTS];   /* each slot's last chunk */
	for (int k = 0; k < HOST_SLOTS; k++)
		pend[k] = UINT64_MAX;

	pthread_mutex_lock(&d->host_lock);
	HIPCHK(hipSetDevice(d->ordinal));
	if ((err = host_staging(d)))
		goto fail;
	/* (registered large slots, a batch of several rounds: zero copy and the
	 * staged gather side by side, host_run_hyb -- off by default, HYB_ST_N) */
	uint64_t hyb_zc = HYB_ZC_CH;
	uint32_t hyb_st = HYB_ST_N;
#ifdef XFG_DIAG
	const char *hz = getenv("XFG_HYB_ZLOG2");   /* zero-copy chunk (log2); 0: no hybrid */
	if (hz && *hz)
		hyb_zc = atoi(hz) ? 1ull << atoi(hz) : 0;
	const char *hn = getenv("XFG_HYB_ST");      /* staged chunks a round */
	if (hn && *hn)
		hyb_st = (uint32_t)atoi(hn);
#endif
	if (zc && hyb_zc && hyb_st && !src->descs && src->stride > HOST_WIN && n >= 2 * hyb_zc &&
	    hyb_zc <= 2 * ZC_CH) {
		err = host_run_hyb(ctx, d, src, n, rbase, verdicts, hyb_zc, hyb_st);
		goto fail;
	}
	if (zc) {
		err = host_run_zc(ctx, d, src, n, rbase, verdicts);
		goto fail;
	}
	for (uint64_t c = 0, k = 0; c < n; c += HOST_CH, k = (k + 1) % HOST_SLOTS) {
		const uint64_t m = n - c < HOST_CH ? n - c : HOST_CH;
		HIPCHK(hipEventSynchronize(d->hs_done[k]));   /* slot k free again */
		if (pend[k] != UINT64_MAX && (err = host_fallback(ctx, d, src, pend[k], k, verdicts)))
			goto fail;
		struct gather_job job = { src, c, m, d->hs_hbuf[k], d->hs_hl[k], stride, whole && !direct };
		if (direct || direct2d)   /* (the slots go by DMA: only the lengths are gathered) */
			job.whole = 2;
		hpool_run(d->pool, gather_slice, &job);
		if (direct2d)
			HIPCHK(hipMemcpy2DAsync(d->hs_dbuf[k], HOST_WIN, src->data + c * src->stride,
						src->stride, HOST_WIN, m, hipMemcpyHostToDevice, d->hs_st[k]));
		else
			HIPCHK(hipMemcpyAsync(d->hs_dbuf[k], direct ? src->data + c * stride : d->hs_hbuf[k],
					      m * stride, hipMemcpyHostToDevice, d->hs_st[k]));
		HIPCHK(hipMemcpyAsync(d->hs_dl[k], d->hs_hl[k], m * 4, hipMemcpyHostToDevice, d->hs_st[k]));
		HIPCHK(hipMemsetAsync(d->hs_fbc[k], 0, 4, d->hs_st[k]));
		struct xfg_batch sub = { d->hs_dbuf[k], NULL, d->hs_dl[k], m, stride, 0 };
		if ((err = host_launch(ctx, d, &sub, d->hs_dv[k], !whole, d->hs_fb[k], d->hs_fbc[k],
				       d->hs_st[k])))
			goto fail;
		HIPCHK(hipMemcpyAsync(verdicts + c, d->hs_dv[k], m, hipMemcpyDeviceToHost, d->hs_st[k]));
		HIPCHK(hipMemcpyAsync(d->hs_hfbc[k], d->hs_fbc[k], 4, hipMemcpyDeviceToHost, d->hs_st[k]));
		HIPCHK(hipEventRecord(d->hs_done[k], d->hs_st[k]));
		pend[k] = whole ? UINT64_MAX : c;
	}
	for (int k = 0; k < HOST_SLOTS; k++) {
		HIPCHK(hipStreamSynchronize(d->hs_st[k]));
		if (pend[k] != UINT64_MAX && (err = host_fallback(ctx, d, src, pend[k], k, verdicts)))
			goto fail;
	}
fail:
	for (int k = 0; k < HOST_SLOTS; k++)   /* (after an error: nothing may still use them) */
		if (d->hs_st[k])
			hipStreamSynchronize(d->hs_st[k]);
	pthread_mutex_unlock(&d->host_lock);
	return err;
}

int xfg_classify_host(xfg_ctx *ctx, int dev, const struct xfg_batch *b, uint8_t *verdicts)
{
	if (!ctx || !b || (!verdicts && b->count) || (b->count && (!b->data || !b->lens)))
		return -EINVAL;
	if (!ctx->ndev)
		return -ENODEV;
	if (dev < 0 || dev >= ctx->ndev)
		return -EINVAL;
	if (!b->offsets && !b->stride && b->count)
		return -EINVAL;
	if (!b->count)
		return 0;
	const struct hsrc src = { b->data, b->offsets, b->stride, b->lens, b->lens_u16, NULL, 0, 0, 0 };
	return host_run(ctx, dev, &src, b->count, verdicts);
}

int xfg_classify_xsk_host(xfg_ctx *ctx, int dev, const struct xfg_desc_batch *b,
			  uint64_t umem_bytes, uint8_t *verdicts)
{
	if (!ctx || !b || (!verdicts && b->count) || (b->count && (!b->umem || !b->descs)))
		return -EINVAL;
	if (!ctx->ndev)
		return -ENODEV;
	if (dev < 0 || dev >= ctx->ndev)
		return -EINVAL;
	if (b->mask != 0xffffffffu && (b->mask & (b->mask + 1)))
		return -EINVAL;   /* a ring mask is 2^k - 1 */
	if (b->count > (uint64_t)b->mask + 1)
		return -EINVAL;
	if (!b->count)
		return 0;
	struct hsrc src = { b->umem, NULL, 0, NULL, 0, b->descs, b->first, b->mask, 0 };
	/* every frame inside the UMEM (the kernel ring would have refused it);
	 * span: the end of the last 16-byte load a kernel makes of a frame */
	for (uint64_t i = 0; i < b->count; i++) {
		const uint64_t a = ((const uint64_t *)b->descs)[2ull * ((b->first + (uint32_t)i) & b->mask)];
		const uint64_t off = (a & ((1ull << 48) - 1)) + (a >> 48);
		const uint32_t l = hsrc_len(&src, i);
		if (off + l > umem_bytes)
			return -EINVAL;
		if (off + ((l + 15ull) & ~15ull) > src.span)
			src.span = off + ((l + 15ull) & ~15ull);
	}
	return host_run(ctx, dev, &src, b->count, verdicts);
}

/* ------------------------------------------------------------------ stats */
int xfg_stats_read_dev(xfg_ctx *ctx, int dev, struct xfg_stats_record out[XFG_ACTION_MAX])
{
	if (!ctx || !out || dev < 0 || dev >= ctx->ndev)
		return -EINVAL;
	struct xfg_dev *d = &ctx->dev[dev];
	unsigned long long s[10];
	int err = dev_read(d, s, ctx->reduced ? d->red_stats : d->stats, sizeof(s));
	if (err)
		return err;
	for (int a = 0; a < XFG_ACTION_MAX; a++) {
		out[a].packets = s[2 * a];
		out[a].bytes = s[2 * a + 1];
	}
	return 0;
}

int xfg_stats_read(xfg_ctx *ctx, struct xfg_stats_record out[XFG_ACTION_MAX])
{
	if (!ctx || !out)
		return -EINVAL;
	memset(out, 0, sizeof(*out) * XFG_ACTION_MAX);
	if (ctx->reduced)   /* every rank holds the job-wide sum already */
		return ctx->ndev ? xfg_stats_read_dev(ctx, 0, out) : 0;
	for (int i = 0; i < ctx->ndev; i++) {
		struct xfg_stats_record r[XFG_ACTION_MAX];
		int err = xfg_stats_read_dev(ctx, i, r);
		if (err)
			return err;
		for (int a = 0; a < XFG_ACTION_MAX; a++) {
			out[a].packets += r[a].packets;
			out[a].bytes += r[a].bytes;
		}
	}
	return 0;
}

int xfg_stats_reset(xfg_ctx *ctx)
{
	if (!ctx)
		return -EINVAL;
	for (int i = 0; i < ctx->ndev; i++) {
		struct xfg_dev *d = &ctx->dev[i];
		unsigned long long z[10] = { 0 };
		int err = dev_write(d, d->stats, z, sizeof(z));
		if (err)
			return err;
	}
	ctx->reduced = 0;
	return 0;
}

int xfg_sync(xfg_ctx *ctx)
{
	if (!ctx)
		return -EINVAL;
	for (int i = 0; i < ctx->ndev; i++) {
		int err = hip_err(hipSetDevice(ctx->dev[i].ordinal));
		if (!err)
			err = hip_err(hipDeviceSynchronize());
		if (err)
			return err;
	}
	return 0;
}

/* ------------------------------------------------------------------ memory */
void *xfg_dev_alloc(xfg_ctx *ctx, int dev, size_t bytes)
{
	void *p = NULL;
	if (!ctx || dev < 0 || dev >= ctx->ndev)
		return NULL;
	if (hipSetDevice(ctx->dev[dev].ordinal) != hipSuccess)
		return NULL;
	if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess)
		return NULL;
	return p;
}

void xfg_dev_free(xfg_ctx *ctx, int dev, void *p)
{
	if (!ctx || dev < 0 || dev >= ctx->ndev || !p)
		return;
	hipSetDevice(ctx->dev[dev].ordinal);
	hipFree(p);
}

int xfg_memcpy_h2d(xfg_ctx *ctx, int dev, void *dst, const void *src, size_t bytes)
{
	if (!ctx || dev < 0 || dev >= ctx->ndev)
		return -EINVAL;
	int err = hip_err(hipSetDevice(ctx->dev[dev].ordinal));
	return err ? err : hip_err(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
}

int xfg_memcpy_d2h(xfg_ctx *ctx, int dev, void *dst, const void *src, size_t bytes)
{
	if (!ctx || dev < 0 || dev >= ctx->ndev)
		return -EINVAL;
	int err = hip_err(hipSetDevice(ctx->dev[dev].ordinal));
	if (!err)
		err = hip_err(hipDeviceSynchronize());
	return err ? err : hip_err(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
}

void *xfg_host_alloc_pinned(size_t bytes)
{
	void *p = NULL;
	if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess)
		return NULL;
	return p;
}

void xfg_host_free_pinned(void *p)
{
	if (p)
		hipHostFree(p);
}

/* ------------------------------------------------------------------ RCCL */
int xfg_comm_unique_id(uint8_t id[XFG_COMM_ID_BYTES])
{
	ncclUniqueId u;
	if (sizeof(u) != XFG_COMM_ID_BYTES)
		return -EINVAL;
	if (ncclGetUniqueId(&u) != ncclSuccess)
		return -EIO;
	memcpy(id, &u, sizeof(u));
	return 0;
}

/* The reduction copies (red_*) and the communicator.  A second init
 * replaces both; a failed init leaves the context without either. */
static void comm_release(xfg_ctx *ctx)
{
	struct xfg_dev *d = &ctx->dev[0];
	if (ctx->comm_ready) {
		ncclCommDestroy(ctx->comm);
		ctx->comm_ready = 0;
	}
	ctx->reduced = 0;
	hipSetDevice(d->ordinal);
	for (int i = 0; i < NMAPS_HASH; i++) {
		hipFree(d->m[i].red_hits);
		d->m[i].red_hits = NULL;
	}
	hipFree(d->red_port_hits);
	d->red_port_hits = NULL;
	hipFree(d->red_stats);
	d->red_stats = NULL;
}

int xfg_comm_init(xfg_ctx *ctx, int nranks, int rank, const uint8_t id[XFG_COMM_ID_BYTES])
{
	int err = 0;
	ncclUniqueId u;
	if (!ctx || !id || ctx->ndev != 1 || nranks < 1 || rank < 0 || rank >= nranks)
		return -EINVAL;
	struct xfg_dev *d = &ctx->dev[0];
	memcpy(&u, id, sizeof(u));
	comm_release(ctx);
	HIPCHK(hipSetDevice(d->ordinal));
	for (int i = 0; i < NMAPS_HASH; i++)
		HIPCHK(hipMalloc((void **)&d->m[i].red_hits, ((size_t)ctx->t[i].nslots + 1) * 8));
	HIPCHK(hipMalloc((void **)&d->red_port_hits, XFG_PORT_MAP_ENTRIES * 8));
	HIPCHK(hipMalloc((void **)&d->red_stats, 10 * 8));
	if (ncclCommInitRank(&ctx->comm, nranks, u, rank) != ncclSuccess) {
		err = -EIO;
		goto fail;
	}
	ctx->comm_ready = 1;
	return 0;
fail:
	comm_release(ctx);
	return err;
}

int xfg_comm_allreduce(xfg_ctx *ctx)
{
	int err = 0;
	if (!ctx || !ctx->comm_ready)
		return -EINVAL;
	struct xfg_dev *d = &ctx->dev[0];
	HIPCHK(hipSetDevice(d->ordinal));
	pthread_mutex_lock(&d->lock);
	err = qt_fold_locked(d);   /* (the QT-order counts into the counters reduced) */
	pthread_mutex_unlock(&d->lock);
	if (err)
		return err;
	HIPCHK(hipStreamSynchronize(d->stream));
	ctx->reduced = 0;
	if (ncclGroupStart() != ncclSuccess)
		return -EIO;
	ncclResult_t r = ncclSuccess;
	for (int i = 0; i < NMAPS_HASH && r == ncclSuccess; i++)
		r = ncclAllReduce(d->m[i].hits, d->m[i].red_hits, (size_t)ctx->t[i].nslots + 1,
				  ncclUint64, ncclSum, ctx->comm, d->stream);
	if (r == ncclSuccess)
		r = ncclAllReduce(d->port_hits, d->red_port_hits, XFG_PORT_MAP_ENTRIES, ncclUint64,
				  ncclSum, ctx->comm, d->stream);
	if (r == ncclSuccess)
		r = ncclAllReduce(d->stats, d->red_stats, 10, ncclUint64, ncclSum, ctx->comm, d->stream);
	/* the group is closed whatever happened inside it */
	const ncclResult_t e = ncclGroupEnd();
	if (r != ncclSuccess || e != ncclSuccess)
		return -EIO;
	HIPCHK(hipStreamSynchronize(d->stream));
	ctx->reduced = 1;
	return 0;
fail:
	return err;
}

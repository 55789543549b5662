/* SPDX-License-Identifier: GPL-2.0 */
/*
 * xfg_plan.c — the launch decision of xfg_classify* (xfg_plan.h).  Each
 * output is assigned once, where all its conditions are known.  The knobs
 * (diagnostics build) are tested as `k && k->...`; the product passes none.
 */
#include "xfg_plan.h"

#include <stdlib.h>
#include <string.h>

#include "xdpfilter_gpu.h"
#include "xfg_table.h"

/* ------------------------------------------------------------------ knobs */
const char *const xfg_knob_names[] = {
	"XFG_WINDOW", "XFG_KERNEL", "XFG_DIAG_MASK", "XFG_TSTAMP", "XFG_BLOOM", "XFG_EMPTY", "XFG_EK",
	"XFG_QT", "XFG_COUNT", "XFG_LOG", "XFG_CW", "XFG_CW_LOG_MIN", "XFG_BLOOM_LDS",
	"XFG_GRID_PER_CU", "XFG_DEFER", "XFG_V6P", "XFG_LOG_PEND", "XFG_QT_DYN_MIN", "XFG_QT_FOLD_AT",
	NULL,
};

void xfg_knobs_init(struct xfg_knobs *k)
{
	memset(k, 0, sizeof(*k));
	k->cw_log_min = XFG_CW_LOG_MIN;
	k->qt_dyn_min = XFG_QT_DYN_MIN;
}

int xfg_knobs_set(struct xfg_knobs *k, const char *name, const char *v)
{
	const int off = !strcmp(v, "off");
	if (!strcmp(name, "XFG_WINDOW"))
		k->window = !strcmp(v, "64") ? 64 : !strcmp(v, "128") ? 128 : 0;
	else if (!strcmp(name, "XFG_KERNEL"))
		k->kernel = !strcmp(v, "general") ? XFG_K_GENERAL : !strcmp(v, "generic") ? XFG_K_GENERIC
			    : !strcmp(v, "split") ? XFG_K_SPLIT : XFG_K_ANY;
	else if (!strcmp(name, "XFG_DIAG_MASK"))
		k->diag_mask = (uint32_t)strtoul(v, NULL, 0);
	else if (!strcmp(name, "XFG_TSTAMP"))
		k->tstamp = strtoull(v, NULL, 0);
	else if (!strcmp(name, "XFG_BLOOM"))
		k->bloom_off = off;
	else if (!strcmp(name, "XFG_EMPTY"))
		k->empty = !strcmp(v, "1");
	else if (!strcmp(name, "XFG_EK"))
		k->ek_off = off;
	else if (!strcmp(name, "XFG_QT"))
		k->qt = off ? XFG_K_QT_OFF : !strcmp(v, "on") ? XFG_K_QT_ON : XFG_K_QT_AUTO;
	else if (!strcmp(name, "XFG_COUNT"))
		k->count_atomic = !strcmp(v, "atomic");
	else if (!strcmp(name, "XFG_LOG"))
		k->log_off = off;
	else if (!strcmp(name, "XFG_CW"))
		k->cw_off = off;
	else if (!strcmp(name, "XFG_CW_LOG_MIN"))
		k->cw_log_min = *v ? strtoull(v, NULL, 0) : XFG_CW_LOG_MIN;
	else if (!strcmp(name, "XFG_BLOOM_LDS"))
		k->bloom_lds_off = off;
	else if (!strcmp(name, "XFG_GRID_PER_CU"))
		k->grid_per_cu = !*v ? 0 : strtol(v, NULL, 0) > 0 ? (uint32_t)strtol(v, NULL, 0) : 1;
	else if (!strcmp(name, "XFG_DEFER"))
		k->defer_kernel = !strcmp(v, "kernel");
	else if (!strcmp(name, "XFG_V6P"))
		k->v6p_off = off;
	else if (!strcmp(name, "XFG_LOG_PEND"))   /* (1: round 4) */
		k->log_pend = !*v ? 0 : strtoul(v, NULL, 0) ? (uint32_t)strtoul(v, NULL, 0) : 1;
	else if (!strcmp(name, "XFG_QT_DYN_MIN"))
		k->qt_dyn_min = *v ? strtoull(v, NULL, 0) : XFG_QT_DYN_MIN;
	else if (!strcmp(name, "XFG_QT_FOLD_AT"))
		k->qt_fold_at = strtoull(v, NULL, 0);
	else
		return -1;
	return 0;
}

/* ------------------------------------------------------------------ helpers */
/* A partition's local-index range of a hit log over @span counters. */
static uint64_t log_hist(uint64_t span)
{
	return ((span + 16 * XFG_LOG_PARTS - 1) / (16 * XFG_LOG_PARTS)) * 16;
}

/* Whether the count kernel covers the hit log of a QT of @span slots: in
 * passes of its LDS histogram (u32 local indices past 65536), or with both
 * lookup directions in one pass (that kernel logs u16 indices only). */
static int qt_log_fits(uint64_t span, int both)
{
	const uint64_t h = log_hist(span);
	return both ? h <= XFG_LOG_HIST_MAX : h <= (uint64_t)XFG_LOG_HIST_MAX * XFG_LOG_PASSES_MAX;
}

/* A persistent grid: @per_cu resident workgroups on every CU, no more than
 * the batch has work for. */
static uint32_t grid_for(const struct xfg_plan_in *in, int per_cu, uint32_t per_wg)
{
	const uint64_t g = (uint64_t)in->ncu * (per_cu > 0 ? per_cu : 1), need = (in->n + per_wg - 1) / per_wg;
	return (uint32_t)(g <= need ? g : need ? need : 1);
}

/* ------------------------------------------------------------------ the kernel */
struct sel {
	uint32_t cnt[3], ports;   /* keys and ruled ports the kernels see (XFG_EMPTY: none) */
	uint32_t gb1, gb3;        /* counter identities: the IPv4 map's, every hash map's */
	uint32_t window, pipe, dense, km, v6d, split, dcnt, qt_live;
	int want_ek, use_ek, use_qt, log_no, kind;
};

static void select_kernel(const struct xfg_plan_in *in, struct sel *s)
{
	const struct xfg_knobs *k = in->knobs;
	const uint32_t f = in->feat;
	const int eth_prog = !(f & (XFG_FEAT_IPV4 | XFG_FEAT_IPV6 | XFG_FEAT_TCP | XFG_FEAT_UDP));
	memset(s, 0, sizeof(*s));
	for (int i = 0; i < 3; i++)
		s->cnt[i] = k && k->empty ? 0 : in->map[i].count;
	s->ports = k && k->empty ? 0 : in->port_count;

	/* Header window: 64 bytes for fixed strides (a parse that reaches past
	 * it -- IPv6/TCP's doff at byte 66, long IPv6 extension chains -- is a
	 * deferred walk over the frame in HBM), unless the context asked for
	 * 128 (xfg_open_opts.window: such frames then stay on the fast path);
	 * frames at offsets stage 128 bytes in the general kernel.  On C4/C5's
	 * 1536-byte slots the 64-byte window was 14 % faster (r04 session 16). */
	uint32_t win = (!in->offsets && in->stride && (in->stride <= 64 || in->ctx_window == 64)) ? 64 : 128;
	if (k && k->window == 64 && !in->offsets && in->stride)
		win = 64;
	else if (k && k->window == 128 && in->stride > 64)
		win = 128;
	/* The pipelined kernels take every fixed-stride batch whose windows can
	 * be loaded without a length (stride >= window, 16-byte aligned; packet
	 * indices fit their 32-bit deferred lists; the per-lane u32 byte sums
	 * bounded), and AF_XDP descriptor batches from descs_min packets (below:
	 * the general kernel's lower fixed cost wins; the descriptor mode sums
	 * in 64 bits) -- except the Ethernet-only programs', whose pipelined
	 * kernel reads fixed-stride slots.  The general kernel the rest: also
	 * the header windows of the host path. */
	int pipe = in->n < (1ull << 32) && !in->hwin && !(k && k->kernel == XFG_K_GENERAL);
	if (in->descs)
		pipe = pipe && !eth_prog && in->n >= in->descs_min;
	else
		pipe = pipe && !in->offsets && in->stride >= win && !(in->stride & 15) && in->aligned16 &&
		       in->stride < 65536 &&
		       (uint64_t)in->stride * (((in->n + 63) / 64 + 1023) / 1024 + 1) < (1ull << 32);
	if (in->descs)   /* (the general kernel: the 128-byte window it always had there) */
		win = pipe ? in->ctx_window : 128;
	s->window = win;
	s->pipe = pipe;
	s->dense = pipe && in->stride == win;

	/* key mode 1: no Ethernet or IPv6 lookup can hit (flag census), so the
	 * pipelined kernel carries IPv4 keys only; never with descriptors */
	const int eth_live = (f & XFG_FEAT_ETHERNET) && in->map[2].count && (in->map[2].fmask & 3);
	const int v6_live = (f & XFG_FEAT_IPV6) && in->map[1].count && (in->map[1].fmask & 3);
	const int v4_prog = !in->descs && (f & XFG_FEAT_IPV4);
	/* (XFG_KERNEL=generic: key mode 0 whatever the census says -- the strided
	 * figure beside a descriptor batch's, tools/bench_configs.py c3d) */
	const int kgen = k && k->kernel == XFG_K_GENERIC;
	const int km4 = v4_prog && !eth_live && !v6_live && !kgen;
	s->split = k && k->kernel == XFG_K_SPLIT && pipe && km4;

	/* The Ethernet map as an LDS key table: the Ethernet-only programs
	 * (kind 6: every lookup answered in LDS, no frame byte past the two
	 * addresses read) and live Ethernet keys beside IP keys (dny_all /
	 * alw_all with a few MAC rules) in the generic and the index kernel. */
	s->want_ek = pipe && (f & XFG_FEAT_ETHERNET) && (eth_prog || eth_live) && !(k && k->ek_off);
	s->use_ek = s->want_ek && in->ek_ok;
	const int eth_kernel = s->use_ek && eth_prog;

	/* small rule sets: a direct LDS counter per hash-map slot (their few
	 * counters are hot: more than the LDS counter cache holds) */
	s->gb1 = in->map[0].nslots + 1;
	s->gb3 = s->gb1 + in->map[1].nslots + 1 + in->map[2].nslots + 1;
	s->dcnt = s->gb3 <= XFG_DCNT_MAX ? s->gb3 : s->gb1 <= XFG_DCNT_MAX ? s->gb1 : 0;
	/* No hit log: a few keys in all -- C1's 8 MAC rules -- are hot (the LDS
	 * counter cache holds every one of them, where the log would send their
	 * hits through a handful of overfull partitions to contended atomics);
	 * every counter has a direct LDS counter; the Ethernet-key kernel
	 * counts in LDS. */
	s->log_no = !pipe || (uint64_t)s->cnt[0] + s->cnt[1] + s->cnt[2] <= XFG_LOG_MIN_KEYS ||
		    s->dcnt >= s->gb3 || eth_kernel || (k && k->count_atomic);

	/* The quotient index (kind 5): one or both IPv4 lookup directions live,
	 * the same flags on every device, a map large enough that the prefilter
	 * + bucket-line chain leaves L2, a hit log the count kernel can take (it
	 * counts through the log only).  Beside it: IPv6 keys (km6: their frames
	 * to the deferred path or, v6p, their lookups in the loop) or Ethernet
	 * keys in the LDS key table (kme).  Without the index the IPv4-key
	 * kernel takes an IPv4-only census, the generic kernel the rest. */
	const int km6 = v4_prog && !eth_live && v6_live;
	const int kme = v4_prog && eth_live && !v6_live && s->use_ek;
	if (pipe && !kgen && (km4 || km6 || kme) && !s->split && !s->log_no) {
		/* (both directions live: up to two images, twice the QT slots) */
		const uint32_t dl = s->cnt[0] && (in->map[0].fmask & 2), sl = s->cnt[0] && (in->map[0].fmask & 1);
		const int ok = (dl | sl) && !in->flags_differ4 &&
			       qt_log_fits(((uint64_t)XFG_QT_SLOTS << xfg_qt_bits_for(s->cnt[0])) << (dl & sl), dl & sl);
		s->use_qt = k && k->qt != XFG_K_QT_AUTO ? ok && k->qt == XFG_K_QT_ON
							 : ok && s->cnt[0] >= in->qt_min_keys;
		s->qt_live = s->use_qt ? (dl ? 2u : 0u) | (sl ? 1u : 0u) : 0;
	}
	s->km = km4 || s->use_qt;
	s->v6d = s->use_qt && km6;
	s->kind = eth_kernel ? XFG_KIND_ETH
		  : !pipe    ? XFG_KIND_GENERAL
		  : !s->km   ? XFG_KIND_PIPE
		  : s->split ? XFG_KIND_SPLIT : s->use_qt ? XFG_KIND_QT : XFG_KIND_IPV4;
}

void xfg_plan_wants(const struct xfg_plan_in *in, struct xfg_wants *w)
{
	struct sel s;
	select_kernel(in, &s);
	w->ek = s.want_ek;
	w->qt_live = s.qt_live;
}

/* ------------------------------------------------------------------ its shape */
/* The count wave: the quotient-index kernel's ninth wave counts the previous
 * launch's log while the others classify, so no count kernel runs between
 * launches -- two sets of slices used in turn; for a 64-byte window, a u16
 * log in one histogram of at most XFG_CW_HIST_MAX (C3's 1M rules: 8192), no
 * IPv6 frames or lookups (@v6) in the loop, no LDS Ethernet table (it and
 * the histogram do not fit beside each other), and the kernel launchable
 * with its histogram. */
static int cw_fits(const struct xfg_plan_in *in, const struct sel *s, uint32_t grid, int occ_c, uint32_t v6)
{
	return log_hist(in->qt_n) <= XFG_CW_HIST_MAX && s->window <= 64 && !v6 && !s->use_ek &&
	       2 * (uint64_t)grid <= XFG_LOG_SLICES_MAX && in->occ[XFG_OCC_CW][0][occ_c] > 0;
}

void xfg_plan(const struct xfg_plan_in *in, struct xfg_plan *p)
{
	const struct xfg_knobs *k = in->knobs;
	struct sel s;
	select_kernel(in, &s);
	memset(p, 0, sizeof(*p));
	p->kind = s.kind;
	p->window = s.window;
	p->pipe = s.pipe;
	p->dense = s.dense;
	p->km = s.km;
	p->v6d = s.v6d;
	p->split = s.split;
	p->use_ek = s.use_ek;
	p->use_qt = s.use_qt;
	p->dcnt = s.dcnt;
	p->bloom_off = k && k->bloom_off && !(in->map[0].count && (in->map[0].fmask & 3) == 3);
	const int wi = s.window > 64, eth_kernel = s.kind == XFG_KIND_ETH;

	/* the generic pipelined kernel: small maps' Bloom filters staged in LDS
	 * (kernel order t4, te, t6; the LDS key table answers the Ethernet
	 * lookups) */
	if (s.pipe && !s.km && !eth_kernel) {
		static const int order[3] = { 0, 2, 1 };
		uint32_t tot = 0;
		for (int i = 0; i < 3; i++) {
			const int m = order[i];
			p->bl_off[i] = ~0u;
			if (s.cnt[m] && in->map[m].bloom_words && !(m == 2 && s.use_ek)) {
				p->bl_off[i] = tot;
				tot += in->map[m].bloom_words;
			}
		}
		if (tot <= XFG_BLOOM_LDS_MAX && !(k && k->bloom_lds_off))
			p->bl_lds = tot;
	}

	const int occ_c = (s.dcnt ? XFG_OCC_DCNT : 0) | (!in->port_tab_ok && s.ports ? XFG_OCC_NIB : 0);
	const int per_cu = k && k->grid_per_cu
		? (int)k->grid_per_cu
		: in->occ[s.kind == XFG_KIND_PIPE && in->descs ? XFG_OCC_DESCS : s.kind][wi]
			 [occ_c | (p->bl_lds ? XFG_OCC_BLOOM : 0) | (s.use_ek ? XFG_OCC_EK : 0)];
	p->per_wg = (uint32_t)in->thr[s.kind][wi];
	p->grid = grid_for(in, per_cu, p->per_wg);
	const uint64_t grid = p->grid, wg_nw = p->per_wg / 64, nt = (in->n + 63) / 64;

	if (s.split) {
		/* the parse pass: its own persistent grid; its records: key a,
		 * ports, key b (both directions live) */
		p->grid_parse = grid_for(in, in->occ[XFG_KIND_SPLIT_PARSE][wi][0], (uint32_t)in->thr[XFG_KIND_SPLIT_PARSE][wi]);
		p->rec_both = s.cnt[0] && (in->map[0].fmask & 3) == 3;
		p->bytes.rec = in->n * 4 * (p->rec_both ? 3 : 2);
	}
	if (s.pipe && !eth_kernel) {   /* (the Ethernet-key kernel defers nothing) */
		/* one deferred list per wave, room for every packet of its tiles --
		 * a quarter more than a fixed share: the quotient-index kernel's
		 * waves take their workgroup's tiles as they go (XFG_QT_DYN), at
		 * most defer_cap / 64 each */
		const uint64_t nw = grid * wg_nw, per = (nt + nw - 1) / nw;
		p->defer_cap = (uint32_t)((per + per / 4 + 2) * 64);
		p->bytes.defer = nw * p->defer_cap * 4;
		/* (XFG_DEFER=kernel: the quotient-index kernel lists its deferred
		 * packets for xfg_defer_kernel, two workgroups a CU over every
		 * list -- 1-3 % slower than each wave's own tail on C3 and C5,
		 * r04 session 19) */
		if (k && k->defer_kernel && s.kind == XFG_KIND_QT && nw <= XFG_DEFER_SRC_MAX) {
			p->defer_sep = 1;
			p->defer_nsrc = (uint32_t)nw;
			p->defer_grid = (uint32_t)in->ncu * 2;
			p->bytes.defer_n = nw * 4;
		}
	}
	/* IPv6 rules beside the index: their lookups in the kernel's loop (1:
	 * one IPv6 direction can hit, one line a frame; 2: both, the src line
	 * beside the dst one), beside one live IPv4 direction or both (the
	 * index never takes both directions with the u32 log: qt_log_fits) */
	if (s.v6d && !(k && k->v6p_off))
		p->v6p = (in->map[1].fmask & 3) == 3 ? 2 : 1;
	/* (the QT kernel's waves taking their workgroup's tiles as they go,
	 * C3 on one box: 2^26 1.059-1.061 against 1.089-1.092 ms, 2^24
	 * 0.294-0.296 against 0.304-0.306, 2^21 equal; C4 at 2^21 1.5 % slower
	 * -- profiles/r06_s13_session.log) */
	p->qt_dyn = s.use_qt && in->n >= (k ? k->qt_dyn_min : XFG_QT_DYN_MIN);
	if (s.use_qt)   /* two halves: the log's counts, the atomics' (xfg_kargs.qt_hitx) */
		p->bytes.qt_hits = (uint64_t)in->qt_n * 8;

	/* Hit log (pipelined kernels): the hash-map counters without a direct
	 * LDS counter -- with the quotient index its QT slots only -- when the
	 * count kernel's histogram covers them (a range past one histogram in
	 * passes) and every workgroup has a slice.  Not for a batch of fewer
	 * packets than counters: the count kernel's pass over every counter
	 * costs more than the atomics it saves -- C5's 15M + 1M rules at 2^23
	 * packets: 0.45 ms with atomics, 0.65-0.71 with the log; C4's 1M at 2^23
	 * and C3's at 2^24 and 2^26 keep the log, r04 sessions 16 and 18.  The
	 * index: from twice as many packets as QT slots (at as many, C3's and
	 * C4's 1M rules at 2^21 packets ran 0.068 / 0.088 ms with the log and
	 * 0.060 / 0.080 without; at twice, the same; at four times, the log
	 * 10 % faster -- profiles/archive/r05_s39_session.log), or, where the
	 * count wave makes the count free, from XFG_CW_LOG_MIN packets (the
	 * atomics it saves are the slow part at C4's per-GPU shard of 2^21). */
	const uint64_t span = s.use_qt ? in->qt_n : (uint64_t)s.gb3 + XFG_PORT_MAP_ENTRIES;
	const uint64_t hist = log_hist(span);
	const uint64_t cw_min = !k ? XFG_CW_LOG_MIN : k->cw_off ? ~0ull : k->cw_log_min;
	const int worth = s.use_qt ? qt_log_fits(span, in->qt_live == 3) &&
					     (2 * span <= in->n || (cw_fits(in, &s, p->grid, occ_c, s.v6d) && in->n >= cw_min))
				   : hist <= (uint64_t)XFG_LOG_HIST_MAX * XFG_LOG_PASSES_MAX && span <= in->n;
	p->logs = !s.log_no && !(k && k->log_off) && grid <= XFG_LOG_SLICES_MAX && worth;
	p->K = 1;
	if (!p->logs)
		return;
	p->log_span = (uint32_t)hist;
	p->log_hist = (uint32_t)(hist < XFG_LOG_HIST_MAX ? hist : XFG_LOG_HIST_MAX);
	p->pwide = hist > 65536;   /* (past 65536 local indices the slices hold u32) */
	/* slice (partition, workgroup): twice a uniform share of the most the
	 * workgroup's waves can log (a fuller one spills to atomics) -- a
	 * workgroup's tiles are a fixed share whichever of its waves takes them */
	const uint64_t wg_all = grid * wg_nw, wg_max = wg_nw * ((nt + wg_all - 1) / wg_all) * 64;
	p->pcap = (uint32_t)((2 * ((wg_max + XFG_LOG_PARTS - 1) / XFG_LOG_PARTS) + 64 + 7) & ~7ull);
	/* the quotient-index kernel's logs of up to K launches side by side in
	 * the partition buffers, counted by one count kernel (its fixed cost
	 * -- a pass over every QT-order count -- paid once per K launches);
	 * every other log is counted after its own launch */
	if (s.use_qt) {
		p->K = k && k->log_pend ? k->log_pend : XFG_LOG_PEND_MAX;
		while (p->K > 1 && p->K * grid > XFG_LOG_SLICES_MAX)
			p->K--;
		/* (measured, profiles/r06_s2_session.log: C3 at 2^24 0.294 against
		 * 0.299 ms a launch; at 2^26 no better -- there the count kernel's
		 * cost is its proportional part, which the count wave pays inside
		 * the launch: it runs below XFG_CW_MAX_PACKETS) */
		p->cw = cw_fits(in, &s, p->grid, occ_c, p->v6p) && in->n < XFG_CW_MAX_PACKETS && !(k && k->cw_off);
		if (p->cw)
			p->K = 2;
	}
	/* (the quotient-index kernel combines its log in LDS and writes the
	 * partition buffers itself: no per-wave regions) */
	p->bytes.tlog = s.use_qt ? 0 : p->bytes.defer;
	p->bytes.pbuf = ((uint64_t)XFG_LOG_PARTS * p->K * grid * p->pcap + 1024) * (p->pwide ? 4 : 2);   /* (+ the count kernel's overread) */
	p->bytes.pfill = (uint64_t)XFG_LOG_PARTS * p->K * grid * 4;
}

/* oracle/ref/ref_forward_harness.c — runs the reference's forwarding programs
 * xdp_fwd_fib_full and xdp_fwd_fib_direct (xdp-forward's xdp_forward.bpf.c,
 * compiled for the host without modification) over a batch of frames: the
 * queue choice and the header rewrite xfg_forward_egress restates.
 *
 * TEST INFRASTRUCTURE ONLY.  Compiled by `make -C oracle ref` into
 * oracle/_ref/libref_forward.so (never committed, never linked by the product).
 * The program text comes from the reference tree at build time; this file and
 * oracle/ref/shim_forward/ hold none of it.
 *
 * What stands in for the kernel:
 *   - bpf_fib_lookup is a brute-force longest-prefix match over the caller's
 *     route list: every route is tried.  The key is ntohl(params->ipv4_dst).
 *     family != AF_INET returns BPF_FIB_LKUP_RET_NOT_FWDED; no covering route
 *     returns NOT_FWDED; a hop with ret != 0 returns that ret; a hop with
 *     mtu != 0 and params->tot_len > mtu returns FRAG_NEEDED (ret before mtu:
 *     the order include/xdpfilter_gpu.h gives; the program returns XDP_PASS
 *     for all of them alike); otherwise it fills ifindex, dmac and smac and
 *     returns 0.  It records the family, tot_len and ipv4_dst it was handed.
 *     The flags (BPF_FIB_LOOKUP_DIRECT) reach nothing else and are ignored.
 *   - bpf_map_lookup_elem(&xdp_tx_ports, &ifindex) is non-NULL if the ifindex
 *     is in the caller's port list, by linear search.
 *   - bpf_redirect_map records its key and returns XDP_REDIRECT.
 *   - ctx->ingress_ifindex is 0.
 *   - frames: the arena of ref_arena.h, as in ref_harness.c.
 *
 * Not thread-safe: call from one thread.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <string.h>

#include "ref_arena.h"

#include "xdp_forward.bpf.c"

enum { REF_FWD_FULL = 0, REF_FWD_DIRECT = 1 };
/* where a frame's run ended */
enum { REF_FWD_ST_EARLY = 0, REF_FWD_ST_NO_ROUTE = 1, REF_FWD_ST_NH_RET = 2, REF_FWD_ST_FRAG = 3,
       REF_FWD_ST_NO_PORT = 4, REF_FWD_ST_REDIRECT = 5, REF_FWD_ST_V6 = 6 };

static const uint32_t *g_routes; /* {prefix (host order), length, next hop} a route */
static uint32_t g_nroutes;
static const uint32_t *g_nh;     /* {ifindex, mtu, ret} a next hop */
static const uint8_t *g_macs;    /* dmac[6], smac[6] a next hop */
static const uint32_t *g_ports;
static uint32_t g_nports;
static uint32_t g_key, g_stage;
static uint32_t g_seen[3];       /* family, tot_len, ipv4_dst as handed to the lookup */

long ref_forward_fib_lookup(void *ctx, void *params, int plen, unsigned int flags)
{
	struct bpf_fib_lookup *p = params;
	(void)ctx;
	(void)flags;
	if (plen != (int)sizeof(*p))
		return -22;
	g_seen[0] = p->family;
	g_seen[1] = p->tot_len;
	g_seen[2] = p->ipv4_dst;
	if (p->family == AF_INET6)
		g_stage = REF_FWD_ST_V6;
	else
		g_stage = REF_FWD_ST_NO_ROUTE;
	if (p->family != AF_INET)
		return BPF_FIB_LKUP_RET_NOT_FWDED;
	const uint32_t key = __builtin_bswap32(p->ipv4_dst);
	int best = -1;
	uint32_t best_len = 0;
	for (uint32_t r = 0; r < g_nroutes; r++) {
		const uint32_t prefix = g_routes[3 * r], len = g_routes[3 * r + 1];
		const uint32_t mask = len ? 0xffffffffu << (32 - len) : 0;
		if ((key & mask) == prefix && (best < 0 || len > best_len)) {
			best = (int)r;
			best_len = len;
		}
	}
	if (best < 0)
		return BPF_FIB_LKUP_RET_NOT_FWDED;
	const uint32_t hop = g_routes[3 * best + 2];
	const uint32_t *h = &g_nh[3 * hop];
	if (h[2]) {
		g_stage = REF_FWD_ST_NH_RET;
		return (long)h[2];
	}
	if (h[1] && p->tot_len > h[1]) {
		g_stage = REF_FWD_ST_FRAG;
		return BPF_FIB_LKUP_RET_FRAG_NEEDED;
	}
	p->ifindex = h[0];
	memcpy(p->dmac, g_macs + 12 * hop, 6);
	memcpy(p->smac, g_macs + 12 * hop + 6, 6);
	g_stage = REF_FWD_ST_NO_PORT; /* until bpf_redirect_map is reached */
	return BPF_FIB_LKUP_RET_SUCCESS;
}

void *ref_forward_port_lookup(const void *map_ptr, const void *key_ptr)
{
	uint32_t k;
	memcpy(&k, key_ptr, sizeof(k));
	if (map_ptr != (const void *)&xdp_tx_ports)
		return NULL;
	for (uint32_t q = 0; q < g_nports; q++)
		if (g_ports[q] == k)
			return (void *)&g_ports[q];
	return NULL;
}

long ref_forward_redirect(const void *map_ptr, unsigned long long key, unsigned long long flags)
{
	(void)map_ptr;
	(void)flags;
	g_key = (uint32_t)key;
	g_stage = REF_FWD_ST_REDIRECT;
	return XDP_REDIRECT;
}

/* Frames as ref_cpumap_run() takes them; mode REF_FWD_FULL or REF_FWD_DIRECT.
 * routes: nroutes {prefix, length, next hop} triples; nh: nnh {ifindex, mtu,
 * ret} triples; macs: 12 bytes a next hop, dmac then smac; ports: the ifindex
 * list of xdp_tx_ports.  Per frame the program's return code in rcs[i], the key
 * it passed to bpf_redirect_map in keys[i] (0xffffffff where it did not
 * redirect), the stage in stages[i], the frame's lens[i] bytes after the run at
 * after + i * after_stride, and in seen[3 * i ..] the family, tot_len and
 * ipv4_dst the lookup was handed (0xffffffff each where it was not called).
 * Returns 0, or -1 for an unknown mode, a route longer than /32 or with bits
 * below its length or an unknown next hop, a frame longer than after_stride,
 * or no arena. */
int ref_forward_run(const uint8_t *data, const uint64_t *offsets, uint32_t stride,
		    const uint32_t *lens, uint64_t n, uint32_t mode,
		    const uint32_t *routes, uint32_t nroutes,
		    const uint32_t *nh, const uint8_t *macs, uint32_t nnh,
		    const uint32_t *ports, uint32_t nports,
		    uint8_t *rcs, uint32_t *keys, uint8_t *stages,
		    uint8_t *after, uint32_t after_stride, uint32_t *seen)
{
	size_t longest = 0;
	for (uint64_t i = 0; i < n; i++)
		if (lens[i] > longest)
			longest = lens[i];
	if (mode > REF_FWD_DIRECT || longest > after_stride)
		return -1;
	for (uint32_t r = 0; r < nroutes; r++) {
		const uint32_t len = routes[3 * r + 1];
		if (len > 32 || routes[3 * r + 2] >= nnh ||
		    (len < 32 && (routes[3 * r] & (0xffffffffu >> len))))
			return -1;
	}
	if (ref_arena_reserve(longest))
		return -1;
	g_routes = routes;
	g_nroutes = nroutes;
	g_nh = nh;
	g_macs = macs;
	g_ports = ports;
	g_nports = nports;

	uint8_t *end = g_arena + g_arena_len;
	for (uint64_t i = 0; i < n; i++) {
		const uint8_t *src = data + (offsets ? offsets[i] : i * (uint64_t)stride);
		uint8_t *dst = end - lens[i];
		memcpy(dst, src, lens[i]);
		struct xdp_md ctx;
		memset(&ctx, 0, sizeof(ctx));
		ctx.data = (uint32_t)(uintptr_t)dst;
		ctx.data_end = (uint32_t)(uintptr_t)end;
		g_key = 0xffffffffu;
		g_stage = REF_FWD_ST_EARLY;
		g_seen[0] = g_seen[1] = g_seen[2] = 0xffffffffu;
		int rc = mode == REF_FWD_FULL ? xdp_fwd_fib_full(&ctx) : xdp_fwd_fib_direct(&ctx);
		rcs[i] = (uint8_t)rc;
		keys[i] = rc == XDP_REDIRECT ? g_key : 0xffffffffu;
		stages[i] = (uint8_t)g_stage;
		memcpy(after + i * (uint64_t)after_stride, dst, lens[i]);
		memcpy(seen + 3 * i, g_seen, sizeof(g_seen));
	}
	g_routes = g_nh = g_ports = NULL;
	g_macs = NULL;
	g_nroutes = g_nports = 0;
	return 0;
}

#ifdef REF_FORWARD_MAIN
/* The stand-alone program of `make -C oracle ref-asan`: this file under ASAN +
 * UBSAN over a batch from a file (tests/fwdrefcorpus.py dump()): u32 magic, n,
 * stride, nroutes, nnh, nports; lens u32[n]; data u8[n * stride]; routes; nh;
 * macs; ports.  Runs both programs and compares them.  Exit status 0; 1 where
 * the run fails or the programs differ; 2 for a file it refuses. */
#include <stdio.h>
#include <stdlib.h>

static void *g_held[24];
static int g_nheld;

static int leave(int rc)
{
	while (g_nheld)
		free(g_held[--g_nheld]);
	return rc;
}

static void *hold(size_t bytes)
{
	void *p = g_nheld < 24 ? malloc(bytes ? bytes : 1) : NULL;
	if (!p) {
		fprintf(stderr, "out of memory\n");
		exit(leave(2));
	}
	g_held[g_nheld++] = p;
	return p;
}

static void *take(FILE *f, size_t bytes)
{
	void *p = hold(bytes);
	if (fread(p, 1, bytes, f) != bytes) {
		fprintf(stderr, "short read\n");
		fclose(f);
		exit(leave(2));
	}
	return p;
}

int main(int argc, char **argv)
{
	FILE *f = argc == 2 ? fopen(argv[1], "rb") : NULL;
	uint32_t h[6];
	if (!f || fread(h, 4, 6, f) != 6 || h[0] != 0x46574452u) {
		fprintf(stderr, "usage: %s batch-file\n", argv[0]);
		if (f)
			fclose(f);
		return 2;
	}
	const uint32_t n = h[1], stride = h[2], nroutes = h[3], nnh = h[4], nports = h[5];
	uint32_t *lens = take(f, 4ull * n);
	uint8_t *data = take(f, (size_t)n * stride);
	uint32_t *routes = take(f, 12ull * nroutes), *nh = take(f, 12ull * nnh);
	uint8_t *macs = take(f, 12ull * nnh);
	uint32_t *ports = take(f, 4ull * nports);
	fclose(f);
	for (uint32_t i = 0; i < n; i++)
		if (lens[i] > stride) {
			fprintf(stderr, "frame %u: %u bytes in a slot of %u\n", i, lens[i], stride);
			return leave(2);
		}
	uint8_t *rcs[2], *stages[2], *after[2];
	uint32_t *keys[2], *seen[2];
	unsigned long hist[7] = { 0 };
	for (int m = 0; m < 2; m++) {
		rcs[m] = hold(n);
		stages[m] = hold(n);
		after[m] = hold((size_t)n * stride);
		keys[m] = hold(4ull * n);
		seen[m] = hold(12ull * n);
		if (ref_forward_run(data, NULL, stride, lens, n, m, routes, nroutes, nh, macs, nnh, ports,
				    nports, rcs[m], keys[m], stages[m], after[m], stride, seen[m])) {
			fprintf(stderr, "ref_forward_run failed\n");
			return leave(1);
		}
	}
	for (uint32_t i = 0; i < n; i++) {
		if (rcs[0][i] != rcs[1][i] || keys[0][i] != keys[1][i] || stages[0][i] != stages[1][i] ||
		    memcmp(after[0] + (size_t)i * stride, after[1] + (size_t)i * stride, lens[i])) {
			fprintf(stderr, "frame %u: full and direct differ\n", i);
			return leave(1);
		}
		hist[stages[0][i] % 7]++;
	}
	printf("%u frames, stages", n);
	for (int s = 0; s < 7; s++)
		printf(" %lu", hist[s]);
	printf("\n");
	return leave(0);
}
#endif

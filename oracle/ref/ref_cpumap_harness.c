/* oracle/ref/ref_cpumap_harness.c — runs the reference's redirect-cpu programs
 * cpumap_l4_hash, cpumap_l4_sport and cpumap_l4_dport (xdp-bench's
 * xdp_redirect_cpumap.bpf.c, compiled for the host without modification) over
 * a batch of frames: the queue choice xfg_steer_egress restates.
 *
 * TEST INFRASTRUCTURE ONLY.  Compiled by `make -C oracle ref` into
 * oracle/_ref/libref_cpumap.so (never committed, never linked by the product).
 * The program text comes from the reference tree at build time; this file and
 * oracle/ref/shim_cpumap/ hold none of it.  The file's other programs
 * (no-touch, touch-data, round-robin, l4-proto, l4-filter, the cpumap and
 * devmap programs) compile along and are never called.
 *
 * What stands in for the kernel:
 *   - cpus_count[0] is the caller's navail; cpus_available[i] the caller's
 *     table, NULL for i >= navail; rx_cnt[0] one struct datarec owned here.
 *     Every other lookup returns NULL.
 *   - bpf_redirect_map records its key and returns XDP_REDIRECT.
 *   - bpf_get_smp_processor_id is 0; nr_cpus is REF_CPUMAP_NR_CPUS.
 *   - frames: the arena of ref_arena.h, as in ref_harness.c.
 *
 * Not thread-safe: call from one thread.
 */
#define _GNU_SOURCE
#include <stdbool.h> /* (the program takes bool from the kernel's headers) */
#include <stdint.h>
#include <string.h>

#include "ref_arena.h"

#include "xdp_redirect_cpumap.bpf.c"

enum { REF_CPUMAP_HASH = 0, REF_CPUMAP_SPORT = 1, REF_CPUMAP_DPORT = 2 };

static const uint32_t *g_avail;
static uint32_t g_navail;
static struct datarec g_rec;
static uint32_t g_key;

void *ref_cpumap_lookup(const void *map_ptr, const void *key_ptr)
{
	uint32_t k;
	memcpy(&k, key_ptr, sizeof(k));
	if (map_ptr == (const void *)&cpus_count)
		return k == 0 ? (void *)&g_navail : NULL;
	if (map_ptr == (const void *)&cpus_available)
		return k < g_navail ? (void *)&g_avail[k] : NULL;
	if (map_ptr == (const void *)&rx_cnt)
		return k == 0 ? (void *)&g_rec : NULL;
	return NULL;
}

long ref_cpumap_redirect(const void *map_ptr, unsigned long long key,
			 unsigned long long flags)
{
	(void)map_ptr;
	(void)flags;
	g_key = (uint32_t)key;
	return XDP_REDIRECT;
}

uint32_t ref_cpumap_nr_cpus(void)
{
	return REF_CPUMAP_NR_CPUS;
}

/* Frames as ref_run() takes them.  Per frame the program's return code in
 * rcs[i] and the key it passed to bpf_redirect_map in keys[i] (0xffffffff
 * where it did not redirect); rec[0] += rx_cnt's processed, rec[1] += its
 * issue.  Returns 0, or -1 for an unknown mode, an empty avail table (the
 * program divides by cpus_count) or no arena. */
int ref_cpumap_run(const uint8_t *data, const uint64_t *offsets, uint32_t stride,
		   const uint32_t *lens, uint64_t n, uint32_t mode,
		   const uint32_t *avail, uint32_t navail,
		   uint8_t *rcs, uint32_t *keys, uint64_t *rec)
{
	size_t longest = 0;
	for (uint64_t i = 0; i < n; i++)
		if (lens[i] > longest)
			longest = lens[i];
	if (mode > REF_CPUMAP_DPORT || !navail || !avail || ref_arena_reserve(longest))
		return -1;
	g_avail = avail;
	g_navail = navail;
	memset(&g_rec, 0, sizeof(g_rec));

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
		int rc = mode == REF_CPUMAP_HASH  ? cpumap_l4_hash(&ctx) :
			 mode == REF_CPUMAP_SPORT ? cpumap_l4_sport(&ctx) :
						    cpumap_l4_dport(&ctx);
		rcs[i] = (uint8_t)rc;
		keys[i] = rc == XDP_REDIRECT ? g_key : 0xffffffffu;
	}
	rec[0] += g_rec.processed;
	rec[1] += g_rec.issue;
	g_avail = NULL;
	g_navail = 0;
	return 0;
}

/* oracle/ref/ref_harness.c — runs one of the reference's xdpfilt_*.c programs,
 * compiled for the host without modification, over a batch of frames.
 *
 * TEST INFRASTRUCTURE ONLY.  Compiled once per variant by `make -C oracle ref`
 * with -DVARIANT_C='"xdpfilt_<variant>.c"' into oracle/_ref/libref_<variant>.so
 * (never committed, never linked by the product).  The program text comes
 * from the reference tree at build time; this file and oracle/ref/shim/ hold
 * none of it.  The entry point is the FUNCNAME the variant file defines.
 *
 * What stands in for the kernel:
 *   - bpf_map_lookup_elem: exact-match key -> pointer to the stored value.
 *     xdp_stats_map and filter_ports are arrays over the caller's storage,
 *     bounds-checked against the map's own max_entries; the three hash maps
 *     are hash indexes over the caller's key and value arrays (the first
 *     occurrence of a duplicate key wins; max_entries is not enforced).
 *   - per-CPU maps: one CPU.
 *   - struct xdp_md's 32-bit data/data_end: every frame is copied into an
 *     arena below 4 GiB so that it ends exactly where a PROT_NONE page
 *     begins; a read past data_end by the program faults here, on the CPU
 *     (ref_arena.h, shared with ref_cpumap_harness.c).
 *
 * Not thread-safe (one arena, one set of map bindings): call from one thread.
 */
#define _GNU_SOURCE
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef VARIANT_C
#error "compile with -DVARIANT_C='\"xdpfilt_<variant>.c\"'"
#endif
#include VARIANT_C

/* ---------------- hash index over caller-owned keys ---------------------- */
struct ref_index {
	const uint8_t *keys;
	uint64_t *vals;
	uint32_t keylen;
	uint32_t *slots; /* rule index + 1, 0 = empty; open addressing */
	uint32_t mask;
};

static uint32_t ref_hash(const uint8_t *k, uint32_t len)
{
	uint64_t h = 0xcbf29ce484222325ull; /* FNV-1a, then a final fold */
	for (uint32_t i = 0; i < len; i++)
		h = (h ^ k[i]) * 0x100000001b3ull;
	return (uint32_t)(h ^ (h >> 29) ^ (h >> 47));
}

static int ref_index_build(struct ref_index *ix, const uint8_t *keys,
			   uint64_t *vals, uint32_t n, uint32_t keylen)
{
	uint32_t cap = 16;
	while (cap < 2 * (uint64_t)n && cap < (1u << 31))
		cap <<= 1;
	if (cap < 2 * (uint64_t)n)
		return -1;
	ix->keys = keys;
	ix->vals = vals;
	ix->keylen = keylen;
	ix->mask = cap - 1;
	ix->slots = calloc(cap, sizeof(uint32_t));
	if (!ix->slots)
		return -1;
	for (uint32_t i = 0; i < n; i++) {
		const uint8_t *k = keys + (size_t)i * keylen;
		uint32_t s = ref_hash(k, keylen) & ix->mask;
		while (ix->slots[s] &&
		       memcmp(keys + (size_t)(ix->slots[s] - 1) * keylen, k, keylen))
			s = (s + 1) & ix->mask;
		if (!ix->slots[s])
			ix->slots[s] = i + 1;
	}
	return 0;
}

static void *ref_index_find(const struct ref_index *ix, const void *key,
			    unsigned long key_size)
{
	if (!ix->slots || key_size != ix->keylen)
		return NULL;
	uint32_t s = ref_hash(key, ix->keylen) & ix->mask;
	for (; ix->slots[s]; s = (s + 1) & ix->mask) {
		uint32_t i = ix->slots[s] - 1;
		if (!memcmp(ix->keys + (size_t)i * ix->keylen, key, ix->keylen))
			return ix->vals + i;
	}
	return NULL;
}

/* ---------------- map storage bound for the current ref_run -------------- */
static struct xdp_stats_record *g_stats; /* [XDP_ACTION_MAX] */
static uint64_t *g_ports;                /* [65536] */
static struct ref_index g_ix4, g_ix6, g_ixe;

static void *ref_array_at(void *base, const void *key, unsigned long key_size,
			  unsigned long max_entries, unsigned long value_size)
{
	uint32_t k;
	if (!base || key_size != sizeof(k))
		return NULL;
	memcpy(&k, key, sizeof(k));
	if (k >= max_entries)
		return NULL;
	return (char *)base + (size_t)k * value_size;
}

void *ref_map_lookup(const void *map_ptr, const void *key_ptr,
		     unsigned long map_type, unsigned long max_entries,
		     unsigned long key_size, unsigned long value_size)
{
	(void)map_type;
	if (map_ptr == (const void *)&xdp_stats_map)
		return ref_array_at(g_stats, key_ptr, key_size, max_entries,
				    value_size);
#if defined(FILT_MODE_TCP) || defined(FILT_MODE_UDP)
	if (map_ptr == (const void *)&filter_ports)
		return ref_array_at(g_ports, key_ptr, key_size, max_entries,
				    value_size);
#endif
#ifdef FILT_MODE_IPV4
	if (map_ptr == (const void *)&filter_ipv4)
		return ref_index_find(&g_ix4, key_ptr, key_size);
#endif
#ifdef FILT_MODE_IPV6
	if (map_ptr == (const void *)&filter_ipv6)
		return ref_index_find(&g_ix6, key_ptr, key_size);
#endif
#ifdef FILT_MODE_ETHERNET
	if (map_ptr == (const void *)&filter_ethernet)
		return ref_index_find(&g_ixe, key_ptr, key_size);
#endif
	abort(); /* a map this harness does not know: the reference changed */
}

/* ---------------- frame arena below 4 GiB, guard page behind it ---------- */
#include "ref_arena.h"

uint32_t ref_features(void)
{
	return _features;
}

/* Frames at data + offsets[i] (or data + i * stride when offsets is NULL),
 * lens[i] bytes each.  Rule values and stats (u64[5][2]: packets, bytes per
 * action) are accumulated in place; one verdict byte per frame.
 * Returns 0, or -1 when the arena or an index cannot be set up. */
int ref_run(const uint8_t *data, const uint64_t *offsets, uint32_t stride,
	    const uint32_t *lens, uint64_t n, uint64_t *ports,
	    const uint8_t *k4, uint64_t *v4, uint32_t n4,
	    const uint8_t *k6, uint64_t *v6, uint32_t n6,
	    const uint8_t *ke, uint64_t *ve, uint32_t ne,
	    uint8_t *verdicts, uint64_t *stats)
{
	int rc = -1;
	size_t longest = 0;
	for (uint64_t i = 0; i < n; i++)
		if (lens[i] > longest)
			longest = lens[i];
	memset(&g_ix4, 0, sizeof(g_ix4));
	memset(&g_ix6, 0, sizeof(g_ix6));
	memset(&g_ixe, 0, sizeof(g_ixe));
	if (ref_arena_reserve(longest) ||
	    ref_index_build(&g_ix4, k4, v4, n4, 4) ||
	    ref_index_build(&g_ix6, k6, v6, n6, 16) ||
	    ref_index_build(&g_ixe, ke, ve, ne, 6))
		goto out;
	g_stats = (struct xdp_stats_record *)stats;
	g_ports = ports;

	uint8_t *end = g_arena + g_arena_len;
	for (uint64_t i = 0; i < n; i++) {
		const uint8_t *src = data + (offsets ? offsets[i] : i * (uint64_t)stride);
		uint8_t *dst = end - lens[i];
		memcpy(dst, src, lens[i]);
		struct xdp_md ctx;
		memset(&ctx, 0, sizeof(ctx));
		ctx.data = (uint32_t)(uintptr_t)dst;
		ctx.data_end = (uint32_t)(uintptr_t)end;
		verdicts[i] = (uint8_t)FUNCNAME(&ctx);
	}
	rc = 0;
out:
	free(g_ix4.slots);
	free(g_ix6.slots);
	free(g_ixe.slots);
	g_ix4.slots = g_ix6.slots = g_ixe.slots = NULL;
	g_stats = NULL;
	g_ports = NULL;
	return rc;
}

/* fib_check.c -- the FIB builder (xdp-tools_amd/csrc/xfg_fib.c) against a
 * brute-force longest-prefix match, as a stand-alone program: tests/test_fib.py
 * builds it with -fsanitize=address,undefined and runs it.
 *
 *   fib_check FILE
 *
 * FILE: "nroutes nnexthops", then nroutes lines "prefix len nexthop" (prefix
 * hexadecimal, host order).  Every next hop gets ifindex 1 + its index.  The
 * program builds the FIB and compares xfg_fib_lookup_host with the brute force
 * on every prefix's first and last address, the addresses just outside, and
 * 20,000 pseudo-random addresses (half of them inside a route).  Prints
 * "ok <lookups>" and exits 0, or prints the first difference and exits 1. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include "xfg_fib.h"

static uint32_t mask_of(unsigned len)
{
	return len ? 0xffffffffu << (32 - len) : 0;
}

static int brute(const struct xfg_fib_route *r, uint64_t n, uint32_t dst, uint32_t *nh)
{
	int best = -1;
	for (uint64_t i = 0; i < n; i++)
		if ((dst & mask_of(r[i].len)) == r[i].prefix && (int)r[i].len > best) {
			best = r[i].len;
			*nh = r[i].nexthop;
		}
	return best < 0 ? -ENOENT : 0;
}

static uint64_t lookups;

static int same(const xfg_fib *f, const struct xfg_fib_route *r, uint64_t n, uint32_t dst)
{
	uint32_t a = 0xdeadbeef, b = 0xdeadbeef;
	const int ea = xfg_fib_lookup_host(f, dst, &a), eb = brute(r, n, dst, &b);
	lookups++;
	if (ea == eb && a == b)
		return 1;
	printf("dst %08x: lookup %d nexthop %u, brute force %d nexthop %u\n", dst, ea, a, eb, b);
	return 0;
}

int main(int argc, char **argv)
{
	unsigned long long nroutes, nnh;
	FILE *in = argc == 2 ? fopen(argv[1], "r") : NULL;
	if (!in || fscanf(in, "%llu %llu", &nroutes, &nnh) != 2)
		return 2;
	struct xfg_fib_route *r = calloc(nroutes ? nroutes : 1, sizeof(*r));
	struct xfg_fib_nexthop *h = calloc(nnh ? nnh : 1, sizeof(*h));
	if (!r || !h)
		return 2;
	for (unsigned long long i = 0; i < nroutes; i++) {
		unsigned prefix, len, nh;
		if (fscanf(in, "%x %u %u", &prefix, &len, &nh) != 3)
			return 2;
		r[i] = (struct xfg_fib_route){ prefix, nh, (uint8_t)len };
	}
	fclose(in);
	for (unsigned long long i = 0; i < nnh; i++)
		h[i].ifindex = 1 + (uint32_t)i;
	xfg_fib *f = NULL;
	const int err = xfg_fib_build_host(r, nroutes, h, (uint32_t)nnh, &f);
	if (err) {
		printf("build: %d\n", err);
		return 1;
	}
	int ok = 1;
	for (unsigned long long i = 0; i < nroutes && ok; i++) {
		const uint32_t first = r[i].prefix, last = r[i].prefix | ~mask_of(r[i].len);
		ok = same(f, r, nroutes, first) && same(f, r, nroutes, last) &&
		     same(f, r, nroutes, first - 1) && same(f, r, nroutes, last + 1);
	}
	uint64_t x = 0x9e3779b97f4a7c15ull;
	for (int k = 0; k < 20000 && ok; k++) {
		x ^= x << 13, x ^= x >> 7, x ^= x << 17;   /* xorshift64 */
		uint32_t dst = (uint32_t)(x >> 16);
		if ((k & 1) && nroutes) {
			const struct xfg_fib_route *in_r = &r[(x >> 48) % nroutes];
			dst = in_r->prefix | (dst & ~mask_of(in_r->len));
		}
		ok = same(f, r, nroutes, dst);
	}
	xfg_fib_free_host(f);
	free(r);
	free(h);
	if (ok)
		printf("ok %llu\n", (unsigned long long)lookups);
	return !ok;
}

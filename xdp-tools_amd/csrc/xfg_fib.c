/* xfg_fib.c -- the builder of the forwarding table (include/xdpfilter_gpu.h,
 * xfg_fib.h): DIR-24-8 with 16-bit entries.  Host code only; the upload is
 * xfg_ctx.c's.
 *
 * The routes are painted in order of ascending length, so a longer prefix
 * overwrites the shorter ones it lies in and every entry ends as its longest
 * match: first the lengths up to 24 into the first table, then the longer
 * ones into second-level groups.  A group is made the first time a /24 gets a
 * longer prefix, filled with that /24's first-table entry -- final by then --
 * which its own entry then gives way to the group's number. */
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include "xfg_fib.h"

struct key {
	uint32_t prefix, nexthop;
	uint8_t len;
};

static int key_cmp(const void *a, const void *b)
{
	const struct key *x = a, *y = b;
	if (x->len != y->len)
		return x->len < y->len ? -1 : 1;
	return x->prefix < y->prefix ? -1 : x->prefix > y->prefix;
}

void xfg_fib_free_host(xfg_fib *fib)
{
	if (!fib)
		return;
	free(fib->t24);
	free(fib->t8);
	free(fib->nh);
	free(fib);
}

int xfg_fib_build_host(const struct xfg_fib_route *routes, uint64_t nroutes,
		       const struct xfg_fib_nexthop *nexthops, uint32_t nnexthops, xfg_fib **out)
{
	if (!out || (nroutes && !routes) || (nnexthops && !nexthops))
		return -EINVAL;
	for (uint64_t i = 0; i < nroutes; i++) {
		const struct xfg_fib_route *r = &routes[i];
		if (r->len > 32 || r->nexthop >= nnexthops)
			return -EINVAL;
		if (r->len < 32 && (r->prefix & (0xffffffffu >> r->len)))
			return -EINVAL;
	}
	for (uint32_t i = 0; i < nnexthops; i++)
		if (!nexthops[i].ifindex)
			return -EINVAL;
	if (nnexthops > XFG_FIB_NEXTHOPS_MAX)
		return -ENOSPC;

	int err = -ENOMEM;
	struct key *k = malloc((nroutes ? nroutes : 1) * sizeof(*k));
	xfg_fib *f = calloc(1, sizeof(*f));
	if (!k || !f)
		goto fail;
	f->dev = -1;
	for (uint64_t i = 0; i < nroutes; i++)
		k[i] = (struct key){ routes[i].prefix, routes[i].nexthop, routes[i].len };
	qsort(k, nroutes, sizeof(*k), key_cmp);
	err = -EEXIST;
	for (uint64_t i = 1; i < nroutes; i++)
		if (k[i].len == k[i - 1].len && k[i].prefix == k[i - 1].prefix)
			goto fail;
	err = -ENOMEM;
	f->t24 = calloc(XFG_FIB_T24_ENTRIES, sizeof(*f->t24));
	if (!f->t24)
		goto fail;
	uint64_t i = 0;
	for (; i < nroutes && k[i].len <= 24; i++) {
		const uint32_t first = k[i].len ? k[i].prefix >> 8 : 0;
		const uint32_t n = 1u << (24 - k[i].len);
		const uint16_t v = (uint16_t)(k[i].nexthop + 1);
		for (uint32_t j = 0; j < n; j++)
			f->t24[first + j] = v;
	}
	uint32_t cap = 0;
	for (; i < nroutes; i++) {
		const uint32_t slot = k[i].prefix >> 8;
		uint16_t e = f->t24[slot];
		if (!(e & XFG_FIB_MORE)) {
			if (f->ngroups == XFG_FIB_GROUPS_MAX) {
				err = -ENOSPC;
				goto fail;
			}
			if (f->ngroups == cap) {
				cap = cap ? 2 * cap : 64;
				uint16_t *t = realloc(f->t8, (size_t)cap * XFG_FIB_GROUP * sizeof(*t));
				if (!t)
					goto fail;
				f->t8 = t;
			}
			uint16_t *g = f->t8 + (size_t)f->ngroups * XFG_FIB_GROUP;
			for (uint32_t j = 0; j < XFG_FIB_GROUP; j++)
				g[j] = e;
			e = f->t24[slot] = (uint16_t)(XFG_FIB_MORE | f->ngroups++);
		}
		uint16_t *g = f->t8 + (size_t)(e & ~XFG_FIB_MORE) * XFG_FIB_GROUP;
		const uint32_t first = k[i].prefix & 0xffu, n = 1u << (32 - k[i].len);
		for (uint32_t j = 0; j < n; j++)
			g[first + j] = (uint16_t)(k[i].nexthop + 1);
	}
	if (!f->t8 && !(f->t8 = calloc(XFG_FIB_GROUP, sizeof(*f->t8))))
		goto fail;
	f->nnh = nnexthops;
	f->nh = calloc(nnexthops ? nnexthops : 1, sizeof(*f->nh));
	if (!f->nh)
		goto fail;
	for (uint32_t j = 0; j < nnexthops; j++) {
		const struct xfg_fib_nexthop *h = &nexthops[j];
		uint8_t mac[12];
		memcpy(mac, h->dmac, 6);
		memcpy(mac + 6, h->smac, 6);
		f->nh[j].ifindex = h->ifindex;
		f->nh[j].mtu_ret = h->mtu | (uint32_t)h->ret << 16;
		memcpy(f->nh[j].mac, mac, 12);
	}
	free(k);
	*out = f;
	return 0;
fail:
	free(k);
	xfg_fib_free_host(f);
	return err;
}

int xfg_fib_lookup_host(const xfg_fib *fib, uint32_t dst, uint32_t *nexthop)
{
	if (!fib || !nexthop)
		return -EINVAL;
	uint16_t e = fib->t24[dst >> 8];
	if (e & XFG_FIB_MORE)
		e = fib->t8[(size_t)(e & ~XFG_FIB_MORE) * XFG_FIB_GROUP + (dst & 0xffu)];
	if (!e)
		return -ENOENT;
	*nexthop = e - 1u;
	return 0;
}

/* xfg_fib.h -- the forwarding table of xfg_forward_egress() as the builder
 * leaves it (xfg_fib.c: host code only, no HIP, so a stand-alone program can
 * link it; tests/fib_check.c does) and as the kernel reads it
 * (xfg_forward.hip).  include/xdpfilter_gpu.h has the format's description. */
#ifndef XFG_FIB_H
#define XFG_FIB_H
#include <stdint.h>
#include "xdpfilter_gpu.h"

#define XFG_FIB_T24_ENTRIES (1u << 24)
#define XFG_FIB_GROUP 256u
#define XFG_FIB_MORE 0x8000u    /* a first-table entry: low 15 bits name a group */

/* A next hop as the kernel loads it, 16 bytes and 4: the three dwords of
 * bytes 0..11 of the rewritten frame follow each other. */
struct xfg_fib_nh {
	uint32_t ifindex;
	uint32_t mtu_ret;           /* mtu | ret << 16 */
	uint32_t mac[3];            /* dmac[0..5], smac[0..5] in memory order */
	uint32_t pad[3];
};

struct xfg_fib {
	xfg_ctx *ctx;               /* the context it was created on */
	int dev;                    /* its device, -1: the host copy only */
	uint32_t ngroups, nnh;
	uint16_t *t24;              /* XFG_FIB_T24_ENTRIES */
	uint16_t *t8;               /* ngroups * XFG_FIB_GROUP (at least one group's room) */
	struct xfg_fib_nh *nh;      /* nnh (at least one record's room) */
	void *d_t24, *d_t8, *d_nh;  /* the device copies */
};

/* The host copy alone: every check of xfg_fib_create() on the routes and next
 * hops, ctx NULL and dev -1 in *out. */
int xfg_fib_build_host(const struct xfg_fib_route *routes, uint64_t nroutes,
		       const struct xfg_fib_nexthop *nexthops, uint32_t nnexthops, xfg_fib **out);
void xfg_fib_free_host(xfg_fib *fib);

#endif

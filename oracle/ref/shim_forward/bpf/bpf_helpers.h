/* oracle/ref/shim_forward/bpf/bpf_helpers.h — host stand-in for libbpf's header
 * of this name, holding only what xdp-forward's kernel program uses of it.
 * This directory goes in front of ../shim/ on the include path of the
 * libref_forward build only; the xdp-filter and redirect-cpu builds never see
 * it (this map carries key_size / value_size, theirs key / value types).
 *
 * TEST INFRASTRUCTURE ONLY.  It lets oracle/ref/ref_forward_harness.c compile
 * the reference's xdp_forward.bpf.c for the host, unmodified.  The stand-ins
 * that carry behaviour are bpf_fib_lookup, bpf_map_lookup_elem and
 * bpf_redirect_map, all three defined in the harness; the rest
 * only makes the declarations parse.
 */
#ifndef XF_REF_SHIM_FORWARD_BPF_HELPERS_H
#define XF_REF_SHIM_FORWARD_BPF_HELPERS_H

/* ELF section placement speaks to the BPF loader only; the host has none. */
#define SEC(section_name)

#ifndef __always_inline
#define __always_inline inline __attribute__((always_inline))
#endif

/* Map attributes are members that are never stored to (see ../../shim/). */
#define __uint(member, number) char (*member)[number]

/* The harness's FIB: fills *params as the kernel helper would and returns a
 * BPF_FIB_LKUP_RET_* code.  @ctx is not read. */
long ref_forward_fib_lookup(void *ctx, void *params, int plen, unsigned int flags);
/* Non-NULL when the int at key_ptr is in the caller's port list. */
void *ref_forward_port_lookup(const void *map_ptr, const void *key_ptr);
/* Records the key; returns XDP_REDIRECT. */
long ref_forward_redirect(const void *map_ptr, unsigned long long key,
			  unsigned long long flags);

#define bpf_fib_lookup(ctx, params, plen, flags) \
	ref_forward_fib_lookup((ctx), (params), (plen), (flags))
#define bpf_map_lookup_elem(map_ptr, key_ptr) \
	ref_forward_port_lookup((const void *)(map_ptr), (key_ptr))
#define bpf_redirect_map(map_ptr, key, flags) \
	ref_forward_redirect((const void *)(map_ptr), (key), (flags))

#endif

/* oracle/ref/shim_cpumap/bpf/bpf_helpers.h — host stand-in for libbpf's header
 * of this name, holding only what xdp-bench's redirect-cpu program and the
 * headers it includes use of it.  This directory goes in front of ../shim/ on
 * the include path of the libref_cpumap build only; the xdp-filter builds
 * never see it (their maps all carry max_entries, these do not).
 *
 * TEST INFRASTRUCTURE ONLY.  It lets oracle/ref/ref_cpumap_harness.c compile
 * the reference's xdp_redirect_cpumap.bpf.c for the host, unmodified.  The
 * stand-ins that carry behaviour are bpf_map_lookup_elem, bpf_redirect_map and
 * bpf_get_smp_processor_id, all three defined in the harness;
 * the rest only makes the declarations parse.
 */
#ifndef XF_REF_SHIM_CPUMAP_BPF_HELPERS_H
#define XF_REF_SHIM_CPUMAP_BPF_HELPERS_H

/* ELF section placement speaks to the BPF loader only; the host has none. */
#define SEC(section_name)

#ifndef __always_inline
#define __always_inline inline __attribute__((always_inline))
#endif

/* Map attributes are members that are never stored to (see ../../shim/). */
#define __uint(member, number) char (*member)[number]
#define __type(member, type_name) __typeof__(type_name) *member

/* The harness's map runtime: the address stored for the u32 at key_ptr in the
 * map object at map_ptr, or NULL. */
void *ref_cpumap_lookup(const void *map_ptr, const void *key_ptr);
/* Records the key; returns XDP_REDIRECT. */
long ref_cpumap_redirect(const void *map_ptr, unsigned long long key,
			 unsigned long long flags);

#define bpf_map_lookup_elem(map_ptr, key_ptr) \
	ref_cpumap_lookup((const void *)(map_ptr), (key_ptr))
#define bpf_redirect_map(map_ptr, key, flags) \
	ref_cpumap_redirect((const void *)(map_ptr), (key), (flags))
#define bpf_get_smp_processor_id() 0u

#endif

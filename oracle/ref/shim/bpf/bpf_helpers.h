/* oracle/ref/shim/bpf/bpf_helpers.h — host stand-in for libbpf's header of
 * this name, holding only what xdp-filter's kernel program uses of it.
 *
 * TEST INFRASTRUCTURE ONLY.  It lets oracle/ref/ref_harness.c compile the
 * reference's xdpfilt_*.c for the host, unmodified.  The one stand-in that
 * carries behaviour is bpf_map_lookup_elem; the rest only
 * makes the declarations parse.
 */
#ifndef XF_REF_SHIM_BPF_HELPERS_H
#define XF_REF_SHIM_BPF_HELPERS_H

/* ELF section placement speaks to the BPF loader only; the host has none. */
#define SEC(section_name)

#ifndef __always_inline
#define __always_inline inline __attribute__((always_inline))
#endif

/* Map attributes are members that are never stored to, only measured:
 * sizeof(*map.max_entries) is the number, sizeof(*map.key) the key type's
 * size.  (The parameter names must not be `key` or `value`: the program
 * passes those as member names.) */
#define __uint(member, number) char (*member)[number]
#define __type(member, type_name) __typeof__(type_name) *member

enum libbpf_pin_type { LIBBPF_PIN_NONE, LIBBPF_PIN_BY_NAME };

/* The harness's map runtime: the address stored for *key_ptr in the map
 * object at map_ptr, or NULL. */
void *ref_map_lookup(const void *map_ptr, const void *key_ptr,
		     unsigned long map_type, unsigned long max_entries,
		     unsigned long key_size, unsigned long value_size);

#define bpf_map_lookup_elem(map_ptr, key_ptr)                               \
	ref_map_lookup((map_ptr), (key_ptr), sizeof(*(map_ptr)->type),      \
		       sizeof(*(map_ptr)->max_entries),                     \
		       sizeof(*(map_ptr)->key), sizeof(*(map_ptr)->value))

#endif

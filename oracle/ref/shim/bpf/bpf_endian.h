/* oracle/ref/shim/bpf/bpf_endian.h — host stand-in for libbpf's header of
 * this name: the two 16-bit byte-order conversions the parsing helpers use.
 * TEST INFRASTRUCTURE ONLY (see bpf_helpers.h beside this file).
 */
#ifndef XF_REF_SHIM_BPF_ENDIAN_H
#define XF_REF_SHIM_BPF_ENDIAN_H

#if __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
#define bpf_htons(x) ((unsigned short)__builtin_bswap16((unsigned short)(x)))
#else
#define bpf_htons(x) ((unsigned short)(x))
#endif
#define bpf_ntohs(x) bpf_htons(x)

#endif

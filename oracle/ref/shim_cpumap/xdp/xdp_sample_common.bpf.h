/* oracle/ref/shim_cpumap/xdp/xdp_sample_common.bpf.h — shadows the reference's
 * header of this name for the libref_cpumap build.
 *
 * TEST INFRASTRUCTURE ONLY.  The real header cannot serve: it defines
 * `const volatile int nr_cpus = 0` (the loader rewrites it before the program
 * is loaded; on the host it would stay 0 and every redirect would be refused),
 * and its tracepoint programs need libbpf's BPF_PROG.  The redirect-cpu
 * programs take two objects from it, both declared by the reference's own
 * xdp_sample.bpf.h (which is compiled as it is): the rx_cnt map and nr_cpus.
 * They are defined here; nr_cpus above every queue number and every port, so
 * that the program's `cpu_dest >= nr_cpus` refuses nothing a test passes.
 */
#ifndef XF_REF_SHIM_CPUMAP_XDP_SAMPLE_COMMON_BPF_H
#define XF_REF_SHIM_CPUMAP_XDP_SAMPLE_COMMON_BPF_H

#include <xdp/xdp_sample.bpf.h>

#define REF_CPUMAP_NR_CPUS (1 << 16)

array_map rx_cnt;
const volatile int nr_cpus = REF_CPUMAP_NR_CPUS;

#endif

/* oracle/ref/shim_cpumap/bpf/bpf_core_read.h — empty on purpose: the
 * redirect-cpu programs use nothing of libbpf's header of this name.
 * TEST INFRASTRUCTURE ONLY. */

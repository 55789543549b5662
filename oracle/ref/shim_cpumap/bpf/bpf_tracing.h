/* oracle/ref/shim_cpumap/bpf/bpf_tracing.h — empty on purpose: the redirect-cpu
 * programs use nothing of libbpf's header of this name (its one user, the
 * tracepoint programs of xdp_sample_common.bpf.h, is shadowed; see
 * ../xdp/xdp_sample_common.bpf.h).  TEST INFRASTRUCTURE ONLY. */

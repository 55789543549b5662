/* steer_hash.c -- a driver for the reference's own xdp-bench/hash_func01.h,
 * compiled by tests/test_steer_model.py with the reference tree's xdp-bench
 * directory on the include path (nothing of the header is copied here).
 * Reads "sum initval" pairs in hex from standard input, a pair a line, and
 * prints SuperFastHash() of the sum's four bytes, as get_ipv4_hash_ip_pair()
 * calls it (xdp-bench/xdp_redirect_cpumap.bpf.c:480-481), one a line. */
#include <stdint.h>
#include <stdio.h>

typedef uint32_t __u32;
typedef uint16_t __u16;
#ifndef __always_inline
#define __always_inline inline __attribute__((always_inline))
#endif

#include "hash_func01.h"

int main(void)
{
	unsigned int sum, initval;
	while (scanf("%x %x", &sum, &initval) == 2) {
		__u32 cpu_hash = sum;
		cpu_hash = SuperFastHash((char *)&cpu_hash, 4, initval);
		printf("%08x\n", cpu_hash);
	}
	return 0;
}

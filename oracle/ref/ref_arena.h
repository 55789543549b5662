/* oracle/ref/ref_arena.h — the frame arena of the reference harnesses
 * (ref_harness.c, ref_cpumap_harness.c): included by each, one arena a
 * library.
 *
 * TEST INFRASTRUCTURE ONLY.  struct xdp_md carries 32-bit data / data_end, so
 * a frame must lie below 4 GiB; and every frame is copied so that it ends
 * exactly where a PROT_NONE page begins: a read past data_end by the program
 * faults here, on the CPU.
 */
#ifndef XF_REF_ARENA_H
#define XF_REF_ARENA_H

#include <stdint.h>
#include <sys/mman.h>
#include <unistd.h>

static uint8_t *g_arena;
static size_t g_arena_len; /* bytes in front of the guard page */

static int ref_arena_reserve(size_t need)
{
	size_t page = (size_t)sysconf(_SC_PAGESIZE);
	size_t len = (need + page - 1) / page * page;
	if (!len)
		len = page;
	if (g_arena && g_arena_len >= len)
		return 0;
	if (g_arena)
		munmap(g_arena, g_arena_len + page);
	g_arena = NULL;
	void *p = mmap(NULL, len + page, PROT_READ | PROT_WRITE,
		       MAP_PRIVATE | MAP_ANONYMOUS | MAP_32BIT, -1, 0);
	if (p == MAP_FAILED)
		return -1;
	if ((uintptr_t)p + len + page > (1ull << 32) ||
	    mprotect((char *)p + len, page, PROT_NONE)) {
		munmap(p, len + page);
		return -1;
	}
	g_arena = p;
	g_arena_len = len;
	return 0;
}

#endif

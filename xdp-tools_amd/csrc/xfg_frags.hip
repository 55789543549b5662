// xfg_frags.hip -- multi-buffer AF_XDP packets (xfg_classify_descs_frags(),
// include/xdpfilter_gpu.h): the head pass over an RX batch whose records may
// carry XDP_PKT_CONTD, and the spread of the per-packet verdicts back over
// the records.  Included by xfg_kernels.hip in the unit with the shared
// kernels.
//
// A packet is a run of records ending at the first one with XDP_PKT_CONTD
// clear (IS_EOP_DESC, lib/util/xdpsock.c:70); a program sees its first record
// only.  The head pass is the tile scan (xfg_scan.hip) over tiles of
// XFG_FRAGS_TILE records with eop = !(options & 1) as the predicate: the
// exclusive prefix sum of the end-of-packet records is the record's packet
// index pkt_of[i].  Record i is a head if i == 0 or record i - 1 ends a
// packet: the neighbouring lane's bit of the same ballot, or for a wave's
// lane 0 one 4-byte load of record i - 1's options.  A head is copied as it
// is to heads[pkt_of[i]], so the packets' first records form a plain
// descriptor array the classify kernels take.  The last tile leaves the
// packet count (its inclusive sum) in state word 2; every tile with an
// end-of-packet record raises state word 3 to its last one's index + 1
// (l2fwd()'s frags_done, lib/util/xdpsock.c:1539-1542).
//
// The spread: verdicts[i] = pv[pkt_of[i]] for the records of complete packets,
// four records a lane (one 16-byte load of packet indices, one 4-byte store),
// from the verdict buffer's first 4-byte boundary; the bytes before it and
// the last few singly.

namespace {
typedef u32x4 __attribute__((aligned(4))) u32x4_a4;
typedef const __attribute__((address_space(1))) u32x4_a4 fr_gidx4;

template <bool NONE>
__device__ __forceinline__ uint32_t fr_verdict(const uint8_t *pv, uint32_t p)
{
	return NONE && p == XFG_SOCKS_FRAGS_PKT_NONE ? XFG_SOCKS_FRAGS_VERDICT_NONE : pv[p];
}

// The launch of a kernel that waits for nothing, 256 threads a workgroup, on
// @stream: a grid of at most @want workgroups (the work's).
template <class K, class... A>
int xfg_flat_launch(K kernel, uint64_t want, unsigned grid, void *stream, const A &...args)
{
	if (grid > want)
		grid = (unsigned)want;
	(void)hipGetLastError();
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), args...);
	return hipGetLastError() == hipSuccess ? 0 : -5;
}
}  // namespace

static_assert(SC_LANES * SC_PASSES == XFG_FRAGS_TILE, "tile shape");

__global__ __launch_bounds__(SC_LANES) void xfg_frags_heads_kernel(const xfg_frags_kargs a)
{
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_base;
	const int tid = threadIdx.x, lane = tid & 63;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_FRAGS_TILES(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 4;
	const uint64_t rx = (uint64_t)(uintptr_t)a.rx, heads = (uint64_t)(uintptr_t)a.heads;
	const uint64_t pko = (uint64_t)(uintptr_t)a.pkt_of;
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_FRAGS_TILE + tid;
		u32x4 rec[SC_PASSES];
		uint32_t prev[SC_PASSES];   // a wave's lane 0: the options of record i - 1
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			rec[k] = u32x4{ 0, 0, 0, XSK_CONTD };   // past the batch: no end of packet
			prev[k] = 0;
			if (i < n)
				rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
					rx + 16ull * ((a.first + (uint32_t)i) & a.mask)));
			if (lane == 0 && i < n && i > 0)
				prev[k] = *reinterpret_cast<gu32 *>(
					rx + 16ull * ((a.first + (uint32_t)i - 1u) & a.mask) + 12);
		}
		// end-of-packet records before this lane's record of pass k: in its wave ...
		uint32_t before[SC_PASSES];
		uint32_t head = 0;      // bit k: the record of pass k starts a packet
		uint32_t last = 0;      // the wave's last end-of-packet record's index + 1
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			const uint64_t b = xfg_wave_rank<false>(!(rec[k].w & XSK_CONTD), k, before[k], s_cnt);
			const bool h = lane ? (b >> (lane - 1)) & 1 : !(prev[k] & XSK_CONTD);
			head |= (uint32_t)(i < n && h) << k;
			if (b)   // (its lanes are inside the batch, below 2^32)
				last = (uint32_t)(i0 - lane + (uint64_t)k * SC_LANES) + 64u -
				       (uint32_t)__builtin_clzll(b);
		}
		__syncthreads();
		// ... and in the tile
		const uint32_t agg = xfg_tile_step<false>(before, s_cnt);
		// the records in complete packets: the wave's last pass with one
		if (lane == 0 && last)
			atomicMax(a.state + 3, (unsigned long long)last);
		// (a tile without an end-of-packet record publishes 0 like any other)
		if (tid == 0) {
			const unsigned long long base = xfg_lookback<false>(status, t, agg);
			s_base = (uint32_t)base;   // (<= n < 2^32)
			if (t == ntiles - 1)
				a.state[2] = base + agg;
		}
		__syncthreads();
		const uint32_t base = s_base;
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			if (i >= n)
				continue;
			const uint32_t p = base + before[k];   // end-of-packet records before i: <= i
			*reinterpret_cast<gu32_w *>(pko + 4ull * i) = p;
			if ((head >> k) & 1)
				*reinterpret_cast<gu32x4_w *>(heads + 16ull * p) = rec[k];
		}
		__syncthreads();   // s_cnt / the ticket's word reused
	}
}

// (NONE: xfg_classify_socks_frags()'s spread over all records, where a record
// of a trailing incomplete packet carries XFG_PKT_NONE and gets
// XFG_VERDICT_NONE)
template <bool NONE>
__global__ __launch_bounds__(256) void xfg_frags_spread_kernel(
	const uint8_t *__restrict__ pv, const uint32_t *__restrict__ pkt_of,
	uint8_t *__restrict__ verdicts, uint32_t done)
{
	const uint64_t vd = (uint64_t)(uintptr_t)verdicts;
	const uint32_t lead = min((uint32_t)(-vd & 3), done);
	const uint32_t groups = (done - lead) / 4;
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t step = gridDim.x * blockDim.x;
	for (uint32_t g = tid; g < groups; g += step) {
		const uint32_t i = lead + 4 * g;
		const u32x4 p = __builtin_nontemporal_load(reinterpret_cast<fr_gidx4 *>(
			(uint64_t)(uintptr_t)pkt_of + 4ull * i));
		*reinterpret_cast<uint32_t *>(verdicts + i) =
			fr_verdict<NONE>(pv, p.x) | fr_verdict<NONE>(pv, p.y) << 8 |
			fr_verdict<NONE>(pv, p.z) << 16 | fr_verdict<NONE>(pv, p.w) << 24;
	}
	// the bytes before the first 4-byte boundary and past the last whole group
	const uint32_t rest = lead + 4 * groups;
	if (tid < lead)
		verdicts[tid] = (uint8_t)fr_verdict<NONE>(pv, pkt_of[tid]);
	if (tid < done - rest)
		verdicts[rest + tid] = (uint8_t)fr_verdict<NONE>(pv, pkt_of[rest + tid]);
}

extern "C" int xfg_launch_frags_heads(const struct xfg_frags_kargs *a, unsigned grid, void *stream)
{
	return xfg_scan_launch(xfg_frags_heads_kernel, a->state, XFG_FRAGS_STATE_WORDS(a->n),
			       XFG_FRAGS_TILES(a->n), grid, static_cast<hipStream_t>(stream), *a);
}

extern "C" int xfg_launch_frags_spread(const uint8_t *pv, const uint32_t *pkt_of, uint8_t *verdicts,
				       uint32_t done, unsigned grid, void *stream)
{
	return xfg_flat_launch(xfg_frags_spread_kernel<false>, ((uint64_t)done / 4 + 255) / 256 + 1, grid,
			       stream, pv, pkt_of, verdicts, done);
}

// xfg_frags.hip -- multi-buffer AF_XDP packets (xfg_classify_descs_frags(),
// include/xdpfilter_gpu.h): the head pass over an RX batch whose records may
// carry XDP_PKT_CONTD, and the spread of the per-packet verdicts back over
// the records.  Included by xfg_kernels.hip in the unit with the shared
// kernels.
//
// A packet is a run of records ending at the first one with XDP_PKT_CONTD
// clear (IS_EOP_DESC, lib/util/xdpsock.c:70); a program sees its first record
// only.  The head pass is the egress kernel's scheme (xfg_egress.hip) with
// eop = !(options & 1) in the place of verdict == PASS: a workgroup takes
// tiles of XFG_FRAGS_TILE records in ticket order, in pass k lane l owns
// record tile * T + k * 256 + l, a ballot gives the end-of-packet records
// before it in its wave and pass, an LDS step those in the tile, a decoupled
// look-back over the earlier tiles' {flag, sum} status words the tile's base.
// That exclusive prefix sum is the record's packet index pkt_of[i].  Record i
// is a head if i == 0 or record i - 1 ends a packet: the neighbouring lane's
// bit of the same ballot, or for a wave's lane 0 one 4-byte load of record
// i - 1's options.  A head is copied as it is to heads[pkt_of[i]], so the
// packets' first records form a plain descriptor array the classify kernels
// take.  The last tile leaves the packet count (its inclusive sum) in state
// word 2; every tile with an end-of-packet record raises state word 3 to its
// last one's index + 1 (l2fwd()'s frags_done, lib/util/xdpsock.c:1539-1542).
//
// The spread: verdicts[i] = pv[pkt_of[i]] for the records of complete packets,
// four records a lane (one 16-byte load of packet indices, one 4-byte store),
// from the verdict buffer's first 4-byte boundary; the bytes before it and
// the last few singly.

namespace {
constexpr int FR_LANES = 256;
constexpr int FR_PASSES = 8;
constexpr int FR_WAVES = FR_LANES / 64;
static_assert(FR_LANES * FR_PASSES == XFG_FRAGS_TILE, "tile shape");
constexpr uint32_t FR_CONTD = 1u;   // XDP_PKT_CONTD, headers/linux/if_xdp.h:123

typedef const __attribute__((address_space(1))) uint32_t fr_gu32;
typedef __attribute__((address_space(1))) uint32_t fr_gu32_w;
typedef __attribute__((address_space(1))) u32x4 fr_gu32x4_w;
typedef u32x4 __attribute__((aligned(4))) u32x4_a4;
typedef const __attribute__((address_space(1))) u32x4_a4 fr_gidx4;
}  // namespace

__global__ __launch_bounds__(FR_LANES) void xfg_frags_heads_kernel(const xfg_frags_kargs a)
{
	__shared__ uint32_t s_cnt[FR_PASSES * FR_WAVES];
	__shared__ uint32_t s_tile, s_base;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_FRAGS_TILES(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 4;
	const uint64_t rx = (uint64_t)(uintptr_t)a.rx, heads = (uint64_t)(uintptr_t)a.heads;
	const uint64_t pko = (uint64_t)(uintptr_t)a.pkt_of;
	for (;;) {
		if (tid == 0)
			s_tile = atomicAdd(ticket, 1u);
		__syncthreads();
		const uint32_t t = s_tile;
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_FRAGS_TILE + tid;
		u32x4 rec[FR_PASSES];
		uint32_t prev[FR_PASSES];   // a wave's lane 0: the options of record i - 1
#pragma unroll
		for (int k = 0; k < FR_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * FR_LANES;
			rec[k] = u32x4{ 0, 0, 0, FR_CONTD };   // past the batch: no end of packet
			prev[k] = 0;
			if (i < n)
				rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
					rx + 16ull * ((a.first + (uint32_t)i) & a.mask)));
			if (lane == 0 && i < n && i > 0)
				prev[k] = *reinterpret_cast<fr_gu32 *>(
					rx + 16ull * ((a.first + (uint32_t)i - 1u) & a.mask) + 12);
		}
		// end-of-packet records before this lane's record of pass k: in its wave ...
		uint32_t before[FR_PASSES];
		uint32_t head = 0;      // bit k: the record of pass k starts a packet
		uint32_t last = 0;      // the wave's last end-of-packet record's index + 1
#pragma unroll
		for (int k = 0; k < FR_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * FR_LANES;
			const uint64_t b = __ballot(!(rec[k].w & FR_CONTD));
			before[k] = __builtin_amdgcn_mbcnt_hi(
				(uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
			const bool h = lane ? (b >> (lane - 1)) & 1 : !(prev[k] & FR_CONTD);
			head |= (uint32_t)(i < n && h) << k;
			if (b)   // (its lanes are inside the batch, below 2^32)
				last = (uint32_t)(i0 - lane + (uint64_t)k * FR_LANES) + 64u -
				       (uint32_t)__builtin_clzll(b);
			if (lane == 0)
				s_cnt[k * FR_WAVES + wave] = __builtin_popcountll(b);
		}
		__syncthreads();
		// ... and in the tile (record order: pass, wave, lane)
		uint32_t agg = 0;
#pragma unroll
		for (int k = 0; k < FR_PASSES; k++) {
#pragma unroll
			for (int w = 0; w < FR_WAVES; w++) {
				if (w == wave)
					before[k] += agg;
				agg += s_cnt[k * FR_WAVES + w];
			}
		}
		// the records in complete packets: the wave's last pass with one
		if (lane == 0 && last)
			atomicMax(a.state + 3, (unsigned long long)last);
		// decoupled look-back (one lane): publish the aggregate, walk back
		// (a tile without an end-of-packet record publishes 0 like any other)
		if (tid == 0) {
			unsigned long long base = 0;
			if (t == 0) {
				__hip_atomic_store(&status[0], CT_INC | agg, __ATOMIC_RELAXED,
						   __HIP_MEMORY_SCOPE_AGENT);
			} else {
				__hip_atomic_store(&status[t], CT_AGG | agg, __ATOMIC_RELAXED,
						   __HIP_MEMORY_SCOPE_AGENT);
				for (uint32_t p = t - 1;;) {
					const unsigned long long w = __hip_atomic_load(
						&status[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (w & CT_INC) {
						base += w & CT_VAL;
						break;
					}
					if (w & CT_AGG) {
						base += w & CT_VAL;
						p--;   // tile 0 always publishes CT_INC
						continue;
					}
					__builtin_amdgcn_s_sleep(1);   // predecessor still counting
				}
				__hip_atomic_store(&status[t], CT_INC | (base + agg), __ATOMIC_RELAXED,
						   __HIP_MEMORY_SCOPE_AGENT);
			}
			s_base = (uint32_t)base;   // (<= n < 2^32)
			if (t == ntiles - 1)
				a.state[2] = base + agg;
		}
		__syncthreads();
		const uint32_t base = s_base;
#pragma unroll
		for (int k = 0; k < FR_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * FR_LANES;
			if (i >= n)
				continue;
			const uint32_t p = base + before[k];   // end-of-packet records before i: <= i
			*reinterpret_cast<fr_gu32_w *>(pko + 4ull * i) = p;
			if ((head >> k) & 1)
				*reinterpret_cast<fr_gu32x4_w *>(heads + 16ull * p) = rec[k];
		}
		__syncthreads();   // s_tile / s_cnt reuse
	}
}

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
			pv[p.x] | (uint32_t)pv[p.y] << 8 | (uint32_t)pv[p.z] << 16 | (uint32_t)pv[p.w] << 24;
	}
	// the bytes before the first 4-byte boundary and past the last whole group
	const uint32_t rest = lead + 4 * groups;
	if (tid < lead)
		verdicts[tid] = pv[pkt_of[tid]];
	if (tid < done - rest)
		verdicts[rest + tid] = pv[pkt_of[rest + tid]];
}

extern "C" int xfg_launch_frags_heads(const struct xfg_frags_kargs *a, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const uint64_t ntiles = XFG_FRAGS_TILES(a->n);
	if (hipMemsetAsync(a->state, 0, XFG_FRAGS_STATE_WORDS(a->n) * 8, s) != hipSuccess)
		return -5;
	if (grid > ntiles)
		grid = (unsigned)ntiles;
	(void)hipGetLastError();
	hipLaunchKernelGGL(xfg_frags_heads_kernel, dim3(grid), dim3(FR_LANES), 0, s, *a);
	return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int xfg_launch_frags_spread(const uint8_t *pv, const uint32_t *pkt_of, uint8_t *verdicts,
				       uint32_t done, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const uint64_t want = ((uint64_t)done / 4 + 255) / 256 + 1;
	if (grid > want)
		grid = (unsigned)want;
	(void)hipGetLastError();
	hipLaunchKernelGGL(xfg_frags_spread_kernel, dim3(grid), dim3(256), 0, s, pv, pkt_of, verdicts,
			   done);
	return hipGetLastError() == hipSuccess ? 0 : -5;
}

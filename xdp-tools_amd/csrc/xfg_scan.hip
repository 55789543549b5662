// xfg_scan.hip -- the tile scan: the device-side pieces every one-pass
// order-preserving kernel of this library is put together from (verdict
// compaction, egress, head passes, capture, and their many-socket forms;
// DESIGN.md §4.12 lists which kernel uses which).  Included by
// xfg_kernels.hip ahead of them, in the unit with the shared kernels.  No
// kernel of its own.
//
// The scheme: a workgroup of SC_LANES lanes takes tiles in ticket order
// (xfg_tile_ticket()); in pass k of SC_PASSES lane l owns item tile * T +
// k * 256 + l, so a wave's loads and its compacted stores are contiguous
// runs.  A ballot ranks an item in its wave and pass (xfg_wave_rank()), an
// LDS step over the (pass, wave) counts in the tile (xfg_tile_step()), and
// one lane's decoupled look-back over the earlier tiles' status words gives
// the tile's base (xfg_lookback(); xfg_lookback_wave() for a tile with K
// sums, a lane a sum).  Kernels that sum bytes instead of
// counting a predicate bring their own wave scan and use the ticket and the
// look-back.
//
// Progress.  A tile waits only for status words of tiles with lower numbers.
// Tile numbers are tickets, so a lower one was drawn earlier, by a workgroup
// that is already running (the launch helper keeps the grid no larger than
// the tile count, its callers no larger than what is resident); what that
// workgroup has to publish needs, in turn, only lower tiles, and its
// aggregate -- enough for a successor to walk past it -- needs none.  Tile 0
// waits for nothing and publishes an inclusive sum.  By induction every wait
// ends.  A kernel that adds waits of its own (the socket kernels' carry and
// counts words) keeps them to words of lower tiles, and the argument holds.

namespace {
constexpr int SC_LANES = 256;
constexpr int SC_PASSES = 8;
constexpr int SC_WAVES = SC_LANES / 64;
constexpr int SC_SLOTS = SC_PASSES * SC_WAVES;   // (pass, wave) pairs: 64 items each

// A status word packs flag (bits 62-63: 1 = the tile's aggregate, 2 = the
// inclusive sum of all tiles up to it) and value, so one 8-byte agent-scope
// atomic carries both and no fence orders anything.
constexpr unsigned long long CT_AGG = 1ull << 62, CT_INC = 2ull << 62, CT_VAL = (1ull << 62) - 1;

constexpr uint64_t XSK_ADDR = (1ull << 48) - 1;   // XSK_UNALIGNED_BUF_ADDR_MASK
constexpr uint32_t XSK_CONTD = 1u;                // XDP_PKT_CONTD, headers/linux/if_xdp.h:123

// global-address-space views (gu32, gu32x4, gdesc: xfg_pipeline.hip)
typedef const __attribute__((address_space(1))) uint8_t gu8;
typedef const __attribute__((address_space(1))) uint16_t gu16;
typedef const __attribute__((address_space(1))) uint64_t gu64;
typedef __attribute__((address_space(1))) uint32_t gu32_w;
typedef __attribute__((address_space(1))) uint64_t gu64_w;
typedef __attribute__((address_space(1))) u32x4 gu32x4_w;
typedef __attribute__((address_space(1))) u32x4_a8 gdesc_w;

// The workgroup's next tile: a ticket drawn by lane 0.  The caller ends its
// loop body with a barrier before it comes here again.
__device__ __forceinline__ uint32_t xfg_tile_ticket(uint32_t *ticket)
{
	__shared__ uint32_t s_tile;
	if (threadIdx.x == 0)
		s_tile = atomicAdd(ticket, 1u);
	__syncthreads();
	return s_tile;
}

// Pass @k's ballot of @p.  @before: the lanes below this one that have it
// set; the wave's count goes to s_cnt[], with KEEP its ballot to s_bal[].
template <bool KEEP>
__device__ __forceinline__ uint64_t xfg_wave_rank(bool p, int k, uint32_t &before, uint32_t *s_cnt,
						  unsigned long long *s_bal = nullptr)
{
	const int slot = k * SC_WAVES + (threadIdx.x >> 6);
	const uint64_t b = __ballot(p);
	before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
					   __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
	if ((threadIdx.x & 63) == 0) {
		if (KEEP)
			s_bal[slot] = b;
		s_cnt[slot] = __builtin_popcountll(b);
	}
	return b;
}

// ... and, after a barrier, the ranks in the tile (item order: pass, wave,
// lane); returns the tile's aggregate.  With KEEP the slots' exclusive prefix
// sums go to s_pre[] (SC_SLOTS + 1 of them), for xfg_tile_before() behind one
// more barrier.
template <bool KEEP>
__device__ __forceinline__ uint32_t xfg_tile_step(uint32_t (&before)[SC_PASSES], const uint32_t *s_cnt,
						  uint32_t *s_pre = nullptr)
{
	const int tid = threadIdx.x, wave = tid >> 6;
	uint32_t agg = 0;
#pragma unroll
	for (int k = 0; k < SC_PASSES; k++) {
#pragma unroll
		for (int w = 0; w < SC_WAVES; w++) {
			if (w == wave)
				before[k] += agg;
			if (KEEP && tid == k * SC_WAVES + w)
				s_pre[tid] = agg;
			agg += s_cnt[k * SC_WAVES + w];
		}
	}
	if (KEEP && tid == SC_SLOTS)
		s_pre[SC_SLOTS] = agg;
	return agg;
}

// The set items of the tile before its position p (0 .. T; any position, not
// only the lane's own; s_bal[SC_SLOTS] is 0, the tile's end).
__device__ __forceinline__ uint32_t xfg_tile_before(const uint32_t *s_pre, const unsigned long long *s_bal,
						    uint32_t p)
{
	return s_pre[p >> 6] + __builtin_popcountll(s_bal[p >> 6] & ((1ull << (p & 63)) - 1));
}

// The decoupled look-back, by one lane: tile @t's aggregate @agg is published
// at once, the sums of the tiles before it collected walking back to the
// first inclusive one, and the tile's own inclusive sum published.  Returns
// the exclusive base.  Relaxed agent-scope atomics: the value travels inside
// the word.  BOUNDED: after XFG_SOCKS_SPINS polls (far past any real wait) it
// gives up with 1 stored to *gave_up rather than hold the device; the base is
// then too small, and still published.
template <bool BOUNDED>
__device__ __forceinline__ unsigned long long xfg_lookback(unsigned long long *status, uint32_t t,
							   unsigned long long agg,
							   unsigned long long *gave_up = nullptr)
{
	unsigned long long base = 0;
	if (t == 0) {
		__hip_atomic_store(&status[0], CT_INC | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return 0;
	}
	__hip_atomic_store(&status[t], CT_AGG | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	[[maybe_unused]] uint32_t spins = 0;
	for (uint32_t p = t - 1;;) {
		const unsigned long long w =
			__hip_atomic_load(&status[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (w & CT_INC) {
			base += w & CT_VAL;
			break;
		}
		if (w & CT_AGG) {
			base += w & CT_VAL;
			p--;   // tile 0 always publishes CT_INC
			continue;
		}
		if constexpr (BOUNDED) {
			if (++spins == XFG_SOCKS_SPINS) {
				__hip_atomic_store(gave_up, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				break;
			}
		}
		__builtin_amdgcn_s_sleep(1);   // predecessor still counting
	}
	__hip_atomic_store(&status[t], CT_INC | (base + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return base;
}

// The look-back over @nq running sums at once, by one wave (the K-way
// partition, xfg_steer.hip): a tile has @nq status words in a row, tile p's
// word of sum q at status[p * nq + q], and lane @q < @nq of the calling wave
// walks sum q's column as xfg_lookback() walks its one -- the tile's aggregate
// published at once, the earlier tiles' collected back to the first inclusive
// word, the tile's own inclusive sum published -- every lane at its own pace,
// so a column whose predecessor is late holds up no other; the lanes' loads of
// one tile's words are one contiguous run.  Returns the lane's exclusive base
// (0 for a lane >= @nq).
__device__ __forceinline__ unsigned long long xfg_lookback_wave(unsigned long long *status, uint32_t nq,
								uint32_t t, uint32_t q,
								unsigned long long agg)
{
	if (q >= nq)
		return 0;
	unsigned long long *col = status + q;
	if (t == 0) {
		__hip_atomic_store(&col[0], CT_INC | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return 0;
	}
	__hip_atomic_store(&col[(uint64_t)t * nq], CT_AGG | agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	unsigned long long base = 0;
	for (uint32_t p = t - 1;;) {
		const unsigned long long w = __hip_atomic_load(&col[(uint64_t)p * nq], __ATOMIC_RELAXED,
							       __HIP_MEMORY_SCOPE_AGENT);
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
	__hip_atomic_store(&col[(uint64_t)t * nq], CT_INC | (base + agg), __ATOMIC_RELAXED,
			   __HIP_MEMORY_SCOPE_AGENT);
	return base;
}

// XFG_EGRESS_SWAP_MACS: bytes 0..5 and 6..11 of the frame at descriptor
// address @addr change places in the UMEM (swap_mac_addresses(),
// lib/util/xdpsock.c:646-654) -- one 16-byte load and store of the frame's
// first 16 bytes (frame starts are 16-byte aligned), bytes 12..15 rewritten
// with their own values.
__device__ __forceinline__ void xfg_swap_macs(uint64_t umem, uint64_t addr)
{
	gu32x4_w *p = reinterpret_cast<gu32x4_w *>(umem + (addr & XSK_ADDR) + (addr >> 48));
	const u32x4 h = *p;
	*p = u32x4{ (h.y >> 16) | (h.z << 16), (h.z >> 16) | (h.x << 16), (h.x >> 16) | (h.y << 16),
		    h.w };
}

// The launch of a tile-scan kernel on @s: its @words state words zeroed first
// (every polled word, every call; 0: a second kernel over words already
// zeroed), a grid of at most @ntiles workgroups.
template <class K, class... A>
int xfg_scan_launch(K kernel, unsigned long long *state, uint64_t words, uint64_t ntiles,
		    unsigned grid, hipStream_t s, const A &...args)
{
	if (words && hipMemsetAsync(state, 0, words * 8, s) != hipSuccess)
		return -5;
	if (grid > ntiles)
		grid = (unsigned)ntiles;
	(void)hipGetLastError();
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(SC_LANES), 0, s, args...);
	return hipGetLastError() == hipSuccess ? 0 : -5;
}
}  // namespace

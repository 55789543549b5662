// xfg_egress.hip -- AF_XDP egress: TX and fill ring records from verdicts
// (xfg_ring_egress(), include/xdpfilter_gpu.h).  Included by xfg_kernels.hip
// in the unit with the shared kernels.
//
// A one-pass, order-preserving two-way partition of an RX descriptor batch:
// the k-th PASS frame's record goes to tx[(tx_first + k) & tx_mask] (addr and
// len as received, options 0: l2fwd(), lib/util/xdpsock.c:1466-1550), the
// j-th other frame's chunk address (addr & (2^48 - 1): xsk_umem__extract_addr(),
// headers/xdp/xsk.h:173-176) to fill[(fill_first + j) & fill_mask] (rx_drop(),
// lib/util/xdpsock.c:1199-1258).
//
// The verdict compaction kernel's scheme (xfg_kernels.hip) over 16-byte
// records: a workgroup takes tiles of XFG_EGRESS_TILE packets in ticket
// order; in pass k lane l of the workgroup owns packet tile * T + k * 256 + l,
// so a wave's record loads are 1 KiB contiguous and its compacted stores
// contiguous runs.  A ballot gives a PASS frame's rank in its wave and pass,
// an LDS step over the (pass, wave) counts its rank in the tile, and a
// decoupled look-back over the earlier tiles' {flag, sum} status words the
// tile's base.  One running sum serves both rings: packet i's fill position
// is i - (PASS frames before i).  A tile waits only for tiles whose tickets
// were drawn before its own, by workgroups already running, so the look-back
// cannot starve (the grid is also no larger than what is resident).
//
// XFG_EGRESS_SWAP_MACS: a PASS frame's bytes 0..5 and 6..11 change places in
// the UMEM (swap_mac_addresses(), lib/util/xdpsock.c:646-654) -- one 16-byte
// load and store of the frame's first 16 bytes (frame starts are 16-byte
// aligned), bytes 12..15 rewritten with their own values.  It depends on the
// verdict alone, so it is issued before the look-back's wait.
//
// XFG_EGRESS_MULTIBUF (multi-buffer packets, every record of one carrying its
// packet's verdict: xfg_classify_descs_frags()): a TX record keeps the RX
// record's XDP_PKT_CONTD (tx_desc->options = eop ? 0 : XDP_PKT_CONTD,
// lib/util/xdpsock.c:1528) and the swap touches a packet's first record only
// (lib/util/xdpsock.c:1521-1522).  The partition itself is the same: it keeps
// the order, so a PASS packet's records stay adjacent on the TX ring.

namespace {
constexpr int EG_LANES = 256;
constexpr int EG_PASSES = 8;
constexpr int EG_WAVES = EG_LANES / 64;
static_assert(EG_LANES * EG_PASSES == XFG_EGRESS_TILE, "tile shape");
constexpr uint64_t EG_ADDR = (1ull << 48) - 1;   // XSK_UNALIGNED_BUF_ADDR_MASK

typedef __attribute__((address_space(1))) u32x4_a8 gdesc_w;
typedef __attribute__((address_space(1))) u32x4 gu32x4_w;
typedef __attribute__((address_space(1))) uint64_t gu64_w;
typedef const __attribute__((address_space(1))) uint8_t gu8;
typedef const __attribute__((address_space(1))) uint32_t eg_gu32;
constexpr uint32_t EG_CONTD = 1u;   // XDP_PKT_CONTD, headers/linux/if_xdp.h:123
}  // namespace

__global__ __launch_bounds__(EG_LANES) void xfg_egress_kernel(const xfg_egress_kargs a)
{
	__shared__ uint32_t s_cnt[EG_PASSES * EG_WAVES];
	__shared__ uint32_t s_tile, s_base;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_EGRESS_TILES(n);
	const bool part = a.tx != nullptr;   // (else every frame to the fill ring)
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 2;
	const uint64_t rx = (uint64_t)(uintptr_t)a.rx, tx = (uint64_t)(uintptr_t)a.tx;
	const uint64_t fill = (uint64_t)(uintptr_t)a.fill, umem = (uint64_t)(uintptr_t)a.umem;
	const uint64_t vd = (uint64_t)(uintptr_t)a.verdicts;
	for (;;) {
		if (tid == 0)
			s_tile = atomicAdd(ticket, 1u);
		__syncthreads();
		const uint32_t t = s_tile;
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_EGRESS_TILE + tid;
		uint32_t vb[EG_PASSES];
		u32x4 rec[EG_PASSES];
#pragma unroll
		for (int k = 0; k < EG_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * EG_LANES;
			vb[k] = 0;
			if (part && i < n)
				vb[k] = *reinterpret_cast<gu8 *>(vd + i);
		}
#pragma unroll
		for (int k = 0; k < EG_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * EG_LANES;
			rec[k] = u32x4{ 0, 0, 0, 0 };
			if (i < n)
				rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
					rx + 16ull * ((a.rx_first + (uint32_t)i) & a.rx_mask)));
		}
		// PASS frames before this lane's packet of pass k: in its wave ...
		uint32_t before[EG_PASSES];
#pragma unroll
		for (int k = 0; k < EG_PASSES; k++) {
			const uint64_t b = __ballot(vb[k] == A_PASS);
			before[k] = __builtin_amdgcn_mbcnt_hi(
				(uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
			if (lane == 0)
				s_cnt[k * EG_WAVES + wave] = __builtin_popcountll(b);
		}
		__syncthreads();
		// ... and in the tile (packet order: pass, wave, lane)
		uint32_t agg = 0;
#pragma unroll
		for (int k = 0; k < EG_PASSES; k++) {
#pragma unroll
			for (int w = 0; w < EG_WAVES; w++) {
				if (w == wave)
					before[k] += agg;
				agg += s_cnt[k * EG_WAVES + w];
			}
		}
		// XFG_EGRESS_MULTIBUF: only a packet's first record is swapped -- record
		// 0, or one whose predecessor has XDP_PKT_CONTD clear (the neighbouring
		// lane's bit of a ballot; a wave's lane 0 loads record i - 1's options)
		uint32_t cont = 0;   // bit k: the record of pass k continues a packet
		if (a.swap_macs && a.multibuf) {
#pragma unroll
			for (int k = 0; k < EG_PASSES; k++) {
				const uint64_t i = i0 + (uint64_t)k * EG_LANES;
				const uint64_t c = __ballot(rec[k].w & EG_CONTD);
				uint32_t prev = (uint32_t)(c >> ((lane - 1) & 63)) & 1;
				if (lane == 0) {
					prev = 0;
					if (i < n && i > 0)
						prev = *reinterpret_cast<eg_gu32 *>(
							rx + 16ull * ((a.rx_first + (uint32_t)i - 1u) & a.rx_mask) +
							12) & EG_CONTD;
				}
				cont |= prev << k;
			}
		}
		if (a.swap_macs) {
#pragma unroll
			for (int k = 0; k < EG_PASSES; k++) {
				if (vb[k] != A_PASS || ((cont >> k) & 1))
					continue;
				const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
				gu32x4_w *p = reinterpret_cast<gu32x4_w *>(umem + (addr & EG_ADDR) +
									   (addr >> 48));
				const u32x4 h = *p;
				*p = u32x4{ (h.y >> 16) | (h.z << 16), (h.z >> 16) | (h.x << 16),
					    (h.x >> 16) | (h.y << 16), h.w };
			}
		}
		// decoupled look-back (one lane): publish the aggregate, walk back
		if (tid == 0) {
			unsigned long long base = 0;
			if (!part) {
				;   // no PASS frame anywhere: nothing to publish or wait for
			} else if (t == 0) {
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
			if (t == ntiles - 1) {
				a.counts[0] = base + agg;
				a.counts[1] = n - (base + agg);
			}
		}
		__syncthreads();
		const uint32_t base = s_base;
		// a TX record's options: 0, or with XFG_EGRESS_MULTIBUF eop ? 0 :
		// XDP_PKT_CONTD (lib/util/xdpsock.c:1528)
		const uint32_t keep = a.multibuf ? EG_CONTD : 0u;
#pragma unroll
		for (int k = 0; k < EG_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * EG_LANES;
			if (i >= n)
				continue;
			const uint32_t np = base + before[k];   // PASS frames before packet i
			if (vb[k] == A_PASS) {
				*reinterpret_cast<gdesc_w *>(tx + 16ull * ((a.tx_first + np) & a.tx_mask)) =
					u32x4{ rec[k].x, rec[k].y, rec[k].z, rec[k].w & keep };
			} else if (fill) {
				const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
				*reinterpret_cast<gu64_w *>(
					fill + 8ull * ((a.fill_first + ((uint32_t)i - np)) & a.fill_mask)) =
					addr & EG_ADDR;
			}
		}
		__syncthreads();   // s_tile / s_cnt reuse
	}
}

extern "C" int xfg_launch_egress(const struct xfg_egress_kargs *a, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const uint64_t ntiles = XFG_EGRESS_TILES(a->n);
	if (hipMemsetAsync(a->state, 0, XFG_EGRESS_STATE_WORDS(a->n) * 8, s) != hipSuccess)
		return -5;
	if (grid > ntiles)
		grid = (unsigned)ntiles;
	(void)hipGetLastError();
	hipLaunchKernelGGL(xfg_egress_kernel, dim3(grid), dim3(EG_LANES), 0, s, *a);
	return hipGetLastError() == hipSuccess ? 0 : -5;
}

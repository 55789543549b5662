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
// The tile scan (xfg_scan.hip) over 16-byte records with verdict == PASS as
// the predicate, tiles of XFG_EGRESS_TILE packets: a wave's record loads are
// 1 KiB contiguous and its compacted stores contiguous runs.  One running sum
// serves both rings: packet i's fill position is i - (PASS frames before i).
//
// XFG_EGRESS_SWAP_MACS (xfg_swap_macs()) depends on the verdict alone, so it
// is issued before the look-back's wait.
//
// XFG_EGRESS_MULTIBUF (multi-buffer packets, every record of one carrying its
// packet's verdict: xfg_classify_descs_frags()): a TX record keeps the RX
// record's XDP_PKT_CONTD (tx_desc->options = eop ? 0 : XDP_PKT_CONTD,
// lib/util/xdpsock.c:1528) and the swap touches a packet's first record only
// (lib/util/xdpsock.c:1521-1522).  The partition itself is the same: it keeps
// the order, so a PASS packet's records stay adjacent on the TX ring.

static_assert(SC_LANES * SC_PASSES == XFG_EGRESS_TILE, "tile shape");

__global__ __launch_bounds__(SC_LANES) void xfg_egress_kernel(const xfg_egress_kargs a)
{
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_base;
	const int tid = threadIdx.x, lane = tid & 63;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_EGRESS_TILES(n);
	const bool part = a.tx != nullptr;   // (else every frame to the fill ring)
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 2;
	const uint64_t rx = (uint64_t)(uintptr_t)a.rx, tx = (uint64_t)(uintptr_t)a.tx;
	const uint64_t fill = (uint64_t)(uintptr_t)a.fill, umem = (uint64_t)(uintptr_t)a.umem;
	const uint64_t vd = (uint64_t)(uintptr_t)a.verdicts;
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_EGRESS_TILE + tid;
		uint32_t vb[SC_PASSES];
		u32x4 rec[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			vb[k] = 0;
			if (part && i < n)
				vb[k] = *reinterpret_cast<gu8 *>(vd + i);
		}
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			rec[k] = u32x4{ 0, 0, 0, 0 };
			if (i < n)
				rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
					rx + 16ull * ((a.rx_first + (uint32_t)i) & a.rx_mask)));
		}
		// PASS frames before this lane's packet of pass k: in its wave ...
		uint32_t before[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++)
			xfg_wave_rank<false>(vb[k] == A_PASS, k, before[k], s_cnt);
		__syncthreads();
		// ... and in the tile
		const uint32_t agg = xfg_tile_step<false>(before, s_cnt);
		// XFG_EGRESS_MULTIBUF: only a packet's first record is swapped -- record
		// 0, or one whose predecessor has XDP_PKT_CONTD clear (the neighbouring
		// lane's bit of a ballot; a wave's lane 0 loads record i - 1's options)
		uint32_t cont = 0;   // bit k: the record of pass k continues a packet
		if (a.swap_macs && a.multibuf) {
#pragma unroll
			for (int k = 0; k < SC_PASSES; k++) {
				const uint64_t i = i0 + (uint64_t)k * SC_LANES;
				const uint64_t c = __ballot(rec[k].w & XSK_CONTD);
				uint32_t prev = (uint32_t)(c >> ((lane - 1) & 63)) & 1;
				if (lane == 0) {
					prev = 0;
					if (i < n && i > 0)
						prev = *reinterpret_cast<gu32 *>(
							rx + 16ull * ((a.rx_first + (uint32_t)i - 1u) & a.rx_mask) +
							12) & XSK_CONTD;
				}
				cont |= prev << k;
			}
		}
		if (a.swap_macs) {
#pragma unroll
			for (int k = 0; k < SC_PASSES; k++) {
				if (vb[k] != A_PASS || ((cont >> k) & 1))
					continue;
				xfg_swap_macs(umem, (uint64_t)rec[k].y << 32 | rec[k].x);
			}
		}
		if (tid == 0) {
			// (no TX ring: no PASS frame anywhere, nothing to publish or wait for)
			const unsigned long long base = part ? xfg_lookback<false>(status, t, agg) : 0;
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
		const uint32_t keep = a.multibuf ? XSK_CONTD : 0u;
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
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
					addr & XSK_ADDR;
			}
		}
		__syncthreads();   // s_cnt / the ticket's word reused
	}
}

extern "C" int xfg_launch_egress(const struct xfg_egress_kargs *a, unsigned grid, void *stream)
{
	return xfg_scan_launch(xfg_egress_kernel, a->state, XFG_EGRESS_STATE_WORDS(a->n),
			       XFG_EGRESS_TILES(a->n), grid, static_cast<hipStream_t>(stream), *a);
}

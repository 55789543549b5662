// xfg_socks_frags.hip -- multi-buffer AF_XDP packets of many sockets over one
// UMEM in one call (xfg_classify_socks_frags(), xfg_socks_frags_egress(),
// include/xdpfilter_gpu.h): xfg_frags.hip's head pass and spread and
// xfg_socks.hip's segmented egress put together.  Included by xfg_kernels.hip
// behind both, in the unit with the shared kernels; the flat order, the table
// of bases in LDS, sk_find(), the tiles and the status words are theirs.
//
// Packets are formed per socket: a socket's record 0 starts one whatever the
// socket before it ended with, and the records behind a socket's last
// end-of-packet record (its trailing incomplete packet, records i >= done[s])
// are processed by nothing.  These lie in the middle of flat order, and
// whether a record is one of them depends on records after it, which no
// look-back sees.  So there are two passes over the records:
//
// Done pass: done[s] = max over socket s's end-of-packet records of their
// index in the socket + 1, by atomicMax on a device array the launch zeroed.
// A wave's 64 records are consecutive in flat order, so their sockets do not
// decrease with the lane: a lane issues the atomic only if the next later lane
// of its wave with an end-of-packet record is in another socket (or there is
// none) -- one atomic per wave and socket.  The pass also writes the flat
// array when the caller wants one.  It waits for nothing.
//
// Head pass (the tile scan, as xfg_frags_heads_kernel), the bases and done[]
// in LDS.  Every end-of-packet record lies in a complete packet and every
// complete packet has one, so the end-of-packet records before flat record i
// are the flat packet index p of a record in a complete packet.  A record is
// a head if it is its socket's record 0 or the record before it in its socket
// ends a packet: the neighbouring lane's ballot bit (that lane holds the same
// socket's record, since this one is not record 0), for a wave's lane 0 one
// 4-byte load of that record's options.  A record with i - base[s] < done[s]
// gets pkt_of[i] = p, and heads[p] if it is a head; any other gets
// XFG_PKT_NONE.  The last tile leaves the packet count in state word 2.
//
// Spread: verdicts[i] = pv[pkt_of[i]], or XFG_VERDICT_NONE where pkt_of[i] is
// XFG_PKT_NONE, over all records: xfg_frags_spread_kernel<true> (xfg_frags.hip).
//
// Egress: xfg_socks_egress_kernel over the live records.  A record is live if
// i - base[s] < done[s] (done[] and its prefix sums dbase[] in LDS beside the
// bases, from the host); a record that is not live counts as nothing, goes to
// no ring, and its verdict byte is not read.  PASS records are live, so np(i)
// and the per-socket TX ranks are as before; a live record's shared fill rank
// is the live records before it, dbase[s] + (i - base[s]), minus np(i).  A TX
// record keeps XDP_PKT_CONTD; the MAC swap touches head records only.
//
// Progress (xfg_scan.hip): the done pass and the spread wait for nothing, the
// head pass's only wait is the look-back, the egress kernel's waits are those
// of xfg_socks_egress_kernel.  Every wait is still bounded by XFG_SOCKS_SPINS
// polls and sets state word 1 when it gives up: the classify call then returns
// -EIO with nothing classified (a look-back that gave up yields a sum too
// small, still an index below n), the egress writes no ring entry from a tile
// whose ranks rest on it.
//
// Not here: sockets over different UMEMs, capture by whole packet.

namespace {
constexpr uint32_t SF_PKT_NONE = XFG_SOCKS_FRAGS_PKT_NONE;

// socket s's RX record j (16 bytes), and its options alone
__device__ __forceinline__ u32x4 sf_rec(const u32x4 rx, uint32_t j)
{
	return __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
		((uint64_t)rx.y << 32 | rx.x) + 16ull * ((rx.z + j) & rx.w)));
}

__device__ __forceinline__ uint32_t sf_opts(const u32x4 rx, uint32_t j)
{
	return *reinterpret_cast<gu32 *>(((uint64_t)rx.y << 32 | rx.x) +
					    16ull * ((rx.z + j) & rx.w) + 12);
}
}  // namespace

__global__ __launch_bounds__(256) void xfg_socks_frags_done_kernel(const xfg_socks_frags_kargs a)
{
	__shared__ uint32_t s_sbase[XFG_SOCKS_TABLE_MAX + 1];
	const int lane = threadIdx.x & 63;
	for (uint32_t s = threadIdx.x; s <= a.nsocks; s += 256)
		s_sbase[s] = *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)a.base + 4ull * s);
	__syncthreads();
	uint32_t *done = reinterpret_cast<uint32_t *>(a.state + XFG_SOCKS_FRAGS_DONE_WORD);
	const uint64_t flat = (uint64_t)(uintptr_t)a.flat;
	const uint64_t step = (uint64_t)gridDim.x * 256;
	// (a wave's lanes hold 64 consecutive records and leave the loop together)
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i - lane < a.n; i += step) {
		uint32_t s = 0, upto = 0;
		bool eop = false;
		if (i < a.n) {
			s = sk_find(s_sbase, a.nsocks, (uint32_t)i);
			const uint32_t j = (uint32_t)i - s_sbase[s];
			const u32x4 rec = sf_rec(sk_ring(a.ents, s, 0), j);
			if (flat)
				*reinterpret_cast<gu32x4_w *>(flat + 16ull * i) = rec;
			eop = !(rec.w & XSK_CONTD);
			upto = j + 1;
		}
		// the next later lane with an end-of-packet record: if it is in this
		// lane's socket, it (or one behind it) raises done[s] further
		const uint64_t b = __ballot(eop);
		const uint64_t later = lane == 63 ? 0 : b >> (lane + 1);
		const int next = later ? lane + 1 + __builtin_ctzll(later) : lane;
		const uint32_t s_next = __shfl(s, next);
		if (eop && (!later || s_next != s))
			atomicMax(&done[s], upto);
	}
}

__global__ __launch_bounds__(SC_LANES) void xfg_socks_frags_heads_kernel(const xfg_socks_frags_kargs a)
{
	__shared__ uint32_t s_sbase[XFG_SOCKS_TABLE_MAX + 1];
	__shared__ uint32_t s_done[XFG_SOCKS_TABLE_MAX];
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_base;
	const int tid = threadIdx.x, lane = tid & 63;
	const uint32_t n = a.n, nsocks = a.nsocks;
	const uint32_t ntiles = (uint32_t)XFG_SOCKS_TILES(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status =
		a.state + XFG_SOCKS_FRAGS_DONE_WORD + XFG_SOCKS_FRAGS_DONE_WORDS(nsocks);
	const uint64_t heads = (uint64_t)(uintptr_t)a.heads, pko = (uint64_t)(uintptr_t)a.pkt_of;
	for (uint32_t s = tid; s <= nsocks; s += SC_LANES)
		s_sbase[s] = *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)a.base + 4ull * s);
	// (the done pass's array: complete when this kernel starts)
	for (uint32_t s = tid; s < nsocks; s += SC_LANES)
		s_done[s] = *reinterpret_cast<gu32 *>(
			(uint64_t)(uintptr_t)(a.state + XFG_SOCKS_FRAGS_DONE_WORD) + 4ull * s);
	for (;;) {
		// (the first ticket's barrier also: the tables are staged)
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_SOCKS_TILE + tid;
		u32x4 rec[SC_PASSES];
		uint32_t prev[SC_PASSES];   // a wave's lane 0: the options of its socket's record before
		uint32_t first = 0;         // bit k: the record of pass k is its socket's record 0
		uint32_t whole = 0;         // bit k: ... lies in a complete packet
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			rec[k] = u32x4{ 0, 0, 0, XSK_CONTD };   // past the batch: no end of packet
			prev[k] = 0;
			if (i < n) {
				const uint32_t s = sk_find(s_sbase, nsocks, (uint32_t)i);
				const uint32_t j = (uint32_t)i - s_sbase[s];
				const u32x4 rx = sk_ring(a.ents, s, 0);
				rec[k] = sf_rec(rx, j);
				first |= (uint32_t)(j == 0) << k;
				whole |= (uint32_t)(j < s_done[s]) << k;
				if (lane == 0 && j > 0)
					prev[k] = sf_opts(rx, j - 1);
			}
		}
		// end-of-packet records before this lane's record of pass k: in its wave ...
		uint32_t before[SC_PASSES];
		uint32_t head = 0;      // bit k: the record of pass k starts a complete packet
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t b = xfg_wave_rank<false>(!(rec[k].w & XSK_CONTD), k, before[k], s_cnt);
			// (not record 0: the lane before holds the same socket's record)
			const bool h = ((first >> k) & 1) ||
				       (lane ? (b >> (lane - 1)) & 1 : !(prev[k] & XSK_CONTD));
			head |= (uint32_t)(h && ((whole >> k) & 1)) << k;
		}
		__syncthreads();
		// ... and in the tile
		const uint32_t agg = xfg_tile_step<false>(before, s_cnt);
		// (a tile without an end-of-packet record publishes 0 like any other)
		if (tid == 0) {
			const unsigned long long base = xfg_lookback<true>(status, t, agg, &a.state[1]);
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
			// end-of-packet records before i: < n for a record in a complete
			// packet (its own end lies at or behind it)
			const uint32_t p = base + before[k];
			*reinterpret_cast<gu32_w *>(pko + 4ull * i) = (whole >> k) & 1 ? p : SF_PKT_NONE;
			if ((head >> k) & 1)
				*reinterpret_cast<gu32x4_w *>(heads + 16ull * p) = rec[k];
		}
		__syncthreads();   // s_cnt / the ticket's word reused
	}
}

__global__ __launch_bounds__(SC_LANES) void xfg_socks_frags_egress_kernel(
	const xfg_socks_frags_egress_kargs a)
{
	__shared__ uint32_t s_sbase[XFG_SOCKS_TABLE_MAX + 1];
	__shared__ uint32_t s_done[XFG_SOCKS_TABLE_MAX];
	__shared__ uint32_t s_dbase[XFG_SOCKS_TABLE_MAX + 1];
	__shared__ unsigned long long s_bal[SC_SLOTS + 1];   // ([SC_SLOTS]: 0, the tile's end)
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_pre[SC_SLOTS + 1];             // s_cnt's exclusive prefix sums
	__shared__ uint32_t s_base, s_carry, s_ok;
	const int tid = threadIdx.x, lane = tid & 63;
	const uint32_t n = a.n, nsocks = a.nsocks;
	const uint32_t ntiles = (uint32_t)XFG_SOCKS_TILES(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 2;
	unsigned long long *pub = status + ntiles;   // nsocks + 1 words
	const uint64_t fill = (uint64_t)(uintptr_t)a.fill, umem = (uint64_t)(uintptr_t)a.umem;
	const uint64_t vd = (uint64_t)(uintptr_t)a.verdicts;
	for (uint32_t s = tid; s <= nsocks; s += SC_LANES) {
		s_sbase[s] = *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)a.base + 4ull * s);
		s_dbase[s] = *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)a.dbase + 4ull * s);
		if (s < nsocks)
			s_done[s] = *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)a.done + 4ull * s);
	}
	if (tid == 0)
		s_bal[SC_SLOTS] = 0;
	for (;;) {
		// (the first ticket's barrier also: the tables are staged)
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		const uint32_t t0 = t * XFG_SOCKS_TILE;   // (< n)
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t0 + tid;
		uint32_t sock[SC_PASSES];
		u32x4 rec[SC_PASSES];
		uint32_t live = 0;   // bit k: the record of pass k lies in a complete packet
		uint32_t pass = 0;   // bit k: ... and goes to its socket's TX ring
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			sock[k] = 0;
			rec[k] = u32x4{ 0, 0, 0, 0 };
			if (i < n) {
				const uint32_t s = sk_find(s_sbase, nsocks, (uint32_t)i);
				const uint32_t j = (uint32_t)i - s_sbase[s];
				const u32x4 tx = sk_ring(a.ents, s, 1);
				sock[k] = s;
				rec[k] = sf_rec(sk_ring(a.ents, s, 0), j);
				if (j < s_done[s]) {
					live |= 1u << k;
					// (a socket without a TX ring: its verdicts are not read)
					if ((tx.x | tx.y) && *reinterpret_cast<gu8 *>(vd + i) == A_PASS)
						pass |= 1u << k;
				}
			}
		}
		// PASS records before this lane's record of pass k: in its wave ...
		uint32_t before[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++)
			xfg_wave_rank<true>((pass >> k) & 1, k, before[k], s_cnt, s_bal);
		__syncthreads();
		// ... and in the tile, with the slots' sums for positions that are not
		// the lane's own
		const uint32_t agg = xfg_tile_step<true>(before, s_cnt, s_pre);
		// the swap touches a packet's first record only: its socket's record 0,
		// or one whose predecessor in the socket has XDP_PKT_CONTD clear (the
		// neighbouring lane's bit of a ballot, which is the same socket's record
		// when this one is not record 0; a wave's lane 0 loads the options)
		if (a.swap_macs) {
#pragma unroll
			for (int k = 0; k < SC_PASSES; k++) {
				const uint64_t i = i0 + (uint64_t)k * SC_LANES;
				const uint64_t c = __ballot(rec[k].w & XSK_CONTD);
				if (!((pass >> k) & 1))
					continue;
				const uint32_t j = (uint32_t)i - s_sbase[sock[k]];
				uint32_t cont = (uint32_t)(c >> ((lane - 1) & 63)) & 1;
				if (j == 0)
					cont = 0;
				else if (lane == 0)
					cont = sf_opts(sk_ring(a.ents, sock[k], 0), j - 1) & XSK_CONTD;
				if (cont)
					continue;
				xfg_swap_macs(umem, (uint64_t)rec[k].y << 32 | rec[k].x);
			}
		}
		if (tid == 0)   // (<= n < 2^32)
			s_base = (uint32_t)xfg_lookback<true>(status, t, agg, &a.state[1]);
		__syncthreads();
		const uint32_t base = s_base;
		// np(base[s]) of the sockets whose base lies in this tile, for the tiles
		// they are carried into and for the counts (the last tile: the bases
		// equal to n too, at position T when the batch fills the tile)
		for (uint32_t s = tid; s <= nsocks; s += SC_LANES) {
			const uint32_t b = s_sbase[s];
			if (b >= t0 && (b - t0 < XFG_SOCKS_TILE || t == ntiles - 1))
				__hip_atomic_store(&pub[s], SK_SET | (base + xfg_tile_before(s_pre, s_bal, b - t0)),
						   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		// the socket carried into the tile, if its first record's starts before it
		if (tid == 0) {
			const uint32_t s = sk_find(s_sbase, nsocks, t0);
			uint32_t ok = 1;
			s_carry = s_sbase[s] < t0 ? sk_wait(&pub[s], a.state, &ok) : 0;
			// (a wait that gave up, here or in a tile this one's sums rest on:
			// the ranks are not to be trusted with a ring's bounds)
			s_ok = ok && !__hip_atomic_load(&a.state[1], __ATOMIC_RELAXED,
							__HIP_MEMORY_SCOPE_AGENT);
		}
		__syncthreads();
		const uint32_t carry = s_carry;
		const bool ok = s_ok;
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			if (i >= n || !ok || !((live >> k) & 1))
				continue;
			const uint32_t s = sock[k], b = s_sbase[s];
			const uint32_t np = base + before[k];   // PASS records before flat record i
			// ... and of them, those in its own socket
			const uint32_t r = np - (b < t0 ? carry : base + xfg_tile_before(s_pre, s_bal, b - t0));
			const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
			if ((pass >> k) & 1) {
				// options: eop ? 0 : XDP_PKT_CONTD (lib/util/xdpsock.c:1528)
				const u32x4 tx = sk_ring(a.ents, s, 1);
				*reinterpret_cast<gdesc_w *>(((uint64_t)tx.y << 32 | tx.x) +
							     16ull * ((tx.z + r) & tx.w)) =
					u32x4{ rec[k].x, rec[k].y, rec[k].z, rec[k].w & XSK_CONTD };
			} else if (fill) {
				// the live records before it, less the PASS ones among them
				*reinterpret_cast<gu64_w *>(
					fill + 8ull * ((a.fill_first + (s_dbase[s] + ((uint32_t)i - b) - np)) &
						       a.fill_mask)) = addr & XSK_ADDR;
			} else {
				const u32x4 fr = sk_ring(a.ents, s, 2);
				if (fr.x | fr.y)
					*reinterpret_cast<gu64_w *>(
						((uint64_t)fr.y << 32 | fr.x) +
						8ull * ((fr.z + (((uint32_t)i - b) - r)) & fr.w)) = addr & XSK_ADDR;
			}
		}
		// the counts: every socket's word is published by now or will be, by a
		// tile with a lower number (this tile's own: before the barrier above)
		if (t == ntiles - 1) {
			for (uint32_t s = tid; s <= nsocks; s += SC_LANES) {
				uint32_t got = 1;
				const uint32_t lo = sk_wait(&pub[s], a.state, &got);
				if (s == nsocks) {
					a.counts[2 * s] = lo;
					a.counts[2 * s + 1] = s_dbase[nsocks] - lo;
				} else {
					const uint32_t sent = sk_wait(&pub[s + 1], a.state, &got) - lo;
					a.counts[2 * s] = sent;
					a.counts[2 * s + 1] = s_done[s] - sent;
				}
			}
		}
		__syncthreads();   // s_cnt / s_bal / the ticket's word reused
	}
}

extern "C" int xfg_launch_socks_frags_heads(const struct xfg_socks_frags_kargs *a, unsigned grid,
					    void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	// (the done pass's array lies in the state words: zeroed ahead of it)
	if (hipMemsetAsync(a->state, 0, XFG_SOCKS_FRAGS_STATE_WORDS(a->n, a->nsocks) * 8, s) !=
	    hipSuccess)
		return -5;
	if (xfg_flat_launch(xfg_socks_frags_done_kernel, ((uint64_t)a->n + 255) / 256, grid, stream, *a))
		return -5;
	return xfg_scan_launch(xfg_socks_frags_heads_kernel, a->state, 0, XFG_SOCKS_TILES(a->n), grid, s,
			       *a);
}

extern "C" int xfg_launch_socks_frags_spread(const uint8_t *pv, const uint32_t *pkt_of,
					     uint8_t *verdicts, uint32_t n, unsigned grid, void *stream)
{
	return xfg_flat_launch(xfg_frags_spread_kernel<true>, ((uint64_t)n / 4 + 255) / 256 + 1, grid,
			       stream, pv, pkt_of, verdicts, n);
}

extern "C" int xfg_launch_socks_frags_egress(const struct xfg_socks_frags_egress_kargs *a,
					     unsigned grid, void *stream)
{
	return xfg_scan_launch(xfg_socks_frags_egress_kernel, a->state,
			       XFG_SOCKS_STATE_WORDS(a->n, a->nsocks), XFG_SOCKS_TILES(a->n), grid,
			       static_cast<hipStream_t>(stream), *a);
}

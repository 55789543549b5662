// xfg_frags_chain.hip -- a chained stage over a multi-buffer batch
// (xfg_classify_descs_frags_chain(), include/xdpfilter_gpu.h): the two
// pre-pass kernels that select the packets an earlier stage passed on and
// leave their head records as a plain descriptor array, and the spread of the
// selected packets' new verdicts over their records.  Included by
// xfg_kernels.hip in the unit with the shared kernels.
//
// Packets are formed as xfg_capture_frags.hip forms them.  Record i is live
// if its verdict byte is not 0xff, and continues if it is live and has
// XDP_PKT_CONTD set.  A record starts a segment if it is not live or record
// i - 1 does not continue; a live segment start is a head.  Every live record
// that is no segment start follows a live record that continues, so a segment
// is one record that is not live, or a head and the live records behind it up
// to and with the first end-of-packet record: a segment holds at most one
// live end-of-packet record, its last, and is a complete packet exactly if it
// holds one.
//
// Both pre-pass kernels are the tile scan (xfg_scan.hip) with a plain sum, so
// a tile waits only for the status words of lower tiles, through
// xfg_lookback() alone.
//
// The record pass, over tiles of XFG_FRAGS_CHAIN_TILE records with the
// segment starts as the predicate: the inclusive prefix sum less one is the
// record's segment seg_of[i].  A head stores its index to head_of_seg[seg], a
// live end-of-packet record to end_of_seg[seg]; the launch filled both with
// ones.  Whether record i - 1 continues is the neighbouring lane's bit of the
// ballot of the continuing records, or for a wave's lane 0 two loads.
//
// The segment pass, over tiles of as many segments (there are at most n; an
// entry past the last segment still holds the launch's ones and is no packet)
// with "complete, and its head's verdict byte in chain_mask" as the predicate:
// the exclusive prefix sum is the packet's place k in the selection, idx[k]
// its head's index, sel[k] the head record as received, rank_of_seg[seg] = k
// (ones for every other segment).  The last tile leaves the selected packets
// in state word 2; every workgroup adds its packets' records to state word 3.
//
// The spread: verdicts[i] = pv[rank_of_seg[seg_of[i]]] where that rank exists,
// four records a lane from the verdict buffer's first 4-byte boundary (one
// 16-byte load of segments, four gathers that fall into one or two lines,
// the dword's old bytes merged in, one 4-byte store; a dword with no selected
// record is neither loaded nor stored); the bytes before the boundary and the
// last few singly.  No record walks its packet in any of the three.

static_assert(SC_LANES * SC_PASSES == XFG_FRAGS_CHAIN_TILE, "tile shape");

__global__ __launch_bounds__(SC_LANES) void xfg_frags_chain_segs_kernel(const xfg_frags_chain_kargs a)
{
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_base;
	const int tid = threadIdx.x, lane = tid & 63;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_FRAGS_CHAIN_TILES(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 4;
	const uint64_t rx = (uint64_t)(uintptr_t)a.descs, vd = (uint64_t)(uintptr_t)a.verdicts;
	const uint64_t segp = (uint64_t)(uintptr_t)(a.seg + XFG_FRAGS_CHAIN_SEG_OF_AT(n));
	const uint64_t headp = (uint64_t)(uintptr_t)(a.seg + XFG_FRAGS_CHAIN_HEAD_AT(n));
	const uint64_t endp = (uint64_t)(uintptr_t)(a.seg + XFG_FRAGS_CHAIN_END_AT(n));
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_FRAGS_CHAIN_TILE + tid;
		uint32_t fl[SC_PASSES];   // 1: live, 2: continues, 4: record i - 1 continues (lane 0)
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			uint32_t v = 0xff;
			fl[k] = 0;
			if (i < n)
				v = *reinterpret_cast<gu8 *>(vd + i);
			if (v != 0xff)
				fl[k] = 1u | (*reinterpret_cast<gu32 *>(
						      rx + 16ull * ((a.first + (uint32_t)i) & a.mask) + 12) &
					      XSK_CONTD) << 1;
			// a wave's lane 0: does record i - 1 continue?
			if (lane == 0 && i < n && i > 0 &&
			    *reinterpret_cast<gu8 *>(vd + i - 1) != 0xff)
				fl[k] |= (*reinterpret_cast<gu32 *>(
						  rx + 16ull * ((a.first + (uint32_t)i - 1u) & a.mask) + 12) &
					  XSK_CONTD) << 2;
		}
		// segment starts before this lane's record of pass k: in its wave ...
		uint32_t before[SC_PASSES];
		uint32_t start = 0;   // bit k: the record of pass k starts a segment
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			const uint64_t bc = __ballot(fl[k] & 2u);
			const bool pc = lane ? (bc >> (lane - 1)) & 1 : fl[k] & 4u;
			// (a record past the batch starts nothing)
			const bool st = i < n && (!(fl[k] & 1u) || !pc);
			start |= (uint32_t)st << k;
			xfg_wave_rank<false>(st, k, before[k], s_cnt);
		}
		__syncthreads();
		// ... and in the tile
		const uint32_t agg = xfg_tile_step<false>(before, s_cnt);
		if (tid == 0)
			s_base = (uint32_t)xfg_lookback<false>(status, t, agg);   // (<= n < 2^32)
		__syncthreads();
		const uint32_t base = s_base;
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			if (i >= n)
				continue;
			// record 0 is a start, so the starts up to and with i are >= 1 and
			// <= i + 1: the segment is below n
			const uint32_t st = (start >> k) & 1;
			const uint32_t seg = base + before[k] + st - 1u;
			*reinterpret_cast<gu32_w *>(segp + 4ull * i) = seg;
			if (st && (fl[k] & 1u))
				*reinterpret_cast<gu32_w *>(headp + 4ull * seg) = (uint32_t)i;
			if ((fl[k] & 3u) == 1u)
				*reinterpret_cast<gu32_w *>(endp + 4ull * seg) = (uint32_t)i;
		}
		__syncthreads();   // s_cnt / the ticket's word reused
	}
}

__global__ __launch_bounds__(SC_LANES) void xfg_frags_chain_select_kernel(const xfg_frags_chain_kargs a)
{
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_base;
	__shared__ unsigned long long s_recs;
	const int tid = threadIdx.x;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_FRAGS_CHAIN_TILES(n);
	unsigned long long *state = a.state + XFG_FRAGS_CHAIN_SET_WORDS(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(state);
	unsigned long long *status = state + 4;
	const uint64_t rx = (uint64_t)(uintptr_t)a.descs, vd = (uint64_t)(uintptr_t)a.verdicts;
	const uint64_t idx = (uint64_t)(uintptr_t)a.idx, sel = (uint64_t)(uintptr_t)a.sel;
	const uint64_t rankp = (uint64_t)(uintptr_t)(a.seg + XFG_FRAGS_CHAIN_RANK_AT(n));
	const uint64_t headp = (uint64_t)(uintptr_t)(a.seg + XFG_FRAGS_CHAIN_HEAD_AT(n));
	const uint64_t endp = (uint64_t)(uintptr_t)(a.seg + XFG_FRAGS_CHAIN_END_AT(n));
	uint64_t recs = 0;   // this lane's selected packets' records
	if (tid == 0)
		s_recs = 0;
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t s0 = (uint64_t)t * XFG_FRAGS_CHAIN_TILE + tid;
		uint32_t h[SC_PASSES], e[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t s = s0 + (uint64_t)k * SC_LANES;
			h[k] = e[k] = XFG_FRAGS_CHAIN_NONE;
			if (s < n) {
				h[k] = __builtin_nontemporal_load(reinterpret_cast<gu32 *>(headp + 4ull * s));
				e[k] = __builtin_nontemporal_load(reinterpret_cast<gu32 *>(endp + 4ull * s));
			}
		}
		// the selected packets' heads as plain descriptors
		u32x4 rec[SC_PASSES];
		uint32_t pick = 0;   // bit k: the segment of pass k is a selected packet
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			rec[k] = u32x4{ 0, 0, 0, 0 };
			// (what the record pass stored is below n; anything else is no packet)
			if (h[k] >= n || e[k] >= n || e[k] < h[k])
				continue;
			const uint32_t v = *reinterpret_cast<gu8 *>(vd + h[k]);
			if (v >= 32 || !((a.chain_mask >> v) & 1))
				continue;
			pick |= 1u << k;
			recs += e[k] - h[k] + 1u;
			rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
				rx + 16ull * ((a.first + h[k]) & a.mask)));
		}
		// selected packets before this lane's segment of pass k: in its wave ...
		uint32_t before[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++)
			xfg_wave_rank<false>((pick >> k) & 1, k, before[k], s_cnt);
		__syncthreads();
		// ... and in the tile
		const uint32_t agg = xfg_tile_step<false>(before, s_cnt);
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
			const uint64_t s = s0 + (uint64_t)k * SC_LANES;
			if (s >= n)
				continue;
			const bool on = (pick >> k) & 1;
			const uint32_t p = base + before[k];   // selected packets before s: <= s
			*reinterpret_cast<gu32_w *>(rankp + 4ull * s) = on ? p : XFG_FRAGS_CHAIN_NONE;
			if (!on)
				continue;
			*reinterpret_cast<gu32_w *>(idx + 4ull * p) = h[k];
			*reinterpret_cast<gu32x4_w *>(sel + 16ull * p) = rec[k];
		}
		__syncthreads();   // s_cnt / the ticket's word reused
	}
	if (recs)
		atomicAdd(&s_recs, (unsigned long long)recs);
	__syncthreads();
	if (tid == 0 && s_recs)
		atomicAdd(a.state + 3, s_recs);
}

namespace {
// the new byte of a record whose segment's rank is @r, or its old one
__device__ __forceinline__ uint32_t fc_byte(const uint8_t *pv, uint32_t r, uint32_t old)
{
	return r == XFG_FRAGS_CHAIN_NONE ? old & 0xffu : pv[r];
}
}  // namespace

// (@seg: seg_of, with rank_of_seg behind it at XFG_FRAGS_CHAIN_RANK_AT)
__global__ __launch_bounds__(256) void xfg_frags_chain_spread_kernel(
	const uint8_t *__restrict__ pv, const uint32_t *__restrict__ seg, uint8_t *verdicts, uint32_t n)
{
	const uint32_t *seg_of = seg + XFG_FRAGS_CHAIN_SEG_OF_AT(n);
	const uint32_t *rank = seg + XFG_FRAGS_CHAIN_RANK_AT(n);
	const uint64_t vd = (uint64_t)(uintptr_t)verdicts;
	const uint32_t lead = min((uint32_t)(-vd & 3), n);
	const uint32_t groups = (n - lead) / 4;
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t step = gridDim.x * blockDim.x;
	for (uint32_t g = tid; g < groups; g += step) {
		const uint32_t i = lead + 4 * g;
		const u32x4 s = __builtin_nontemporal_load(reinterpret_cast<fr_gidx4 *>(
			(uint64_t)(uintptr_t)seg_of + 4ull * i));
		const uint32_t r0 = rank[s.x], r1 = rank[s.y], r2 = rank[s.z], r3 = rank[s.w];
		if ((r0 & r1 & r2 & r3) == XFG_FRAGS_CHAIN_NONE)
			continue;
		uint32_t *w = reinterpret_cast<uint32_t *>(verdicts + i);
		const uint32_t old = *w;
		*w = fc_byte(pv, r0, old) | fc_byte(pv, r1, old >> 8) << 8 |
		     fc_byte(pv, r2, old >> 16) << 16 | fc_byte(pv, r3, old >> 24) << 24;
	}
	// the bytes before the first 4-byte boundary and past the last whole group
	const uint32_t rest = lead + 4 * groups;
	if (tid < lead) {
		const uint32_t r = rank[seg_of[tid]];
		if (r != XFG_FRAGS_CHAIN_NONE)
			verdicts[tid] = pv[r];
	}
	if (tid < n - rest) {
		const uint32_t r = rank[seg_of[rest + tid]];
		if (r != XFG_FRAGS_CHAIN_NONE)
			verdicts[rest + tid] = pv[r];
	}
}

extern "C" int xfg_launch_frags_chain_select(const struct xfg_frags_chain_kargs *a, unsigned grid,
					     void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const uint64_t ntiles = XFG_FRAGS_CHAIN_TILES(a->n);
	if (hipMemsetAsync(a->seg + XFG_FRAGS_CHAIN_HEAD_AT(a->n), 0xff, 8ull * a->n, s) != hipSuccess)
		return -5;
	// (both kernels' state words zeroed ahead of the first)
	const int err = xfg_scan_launch(xfg_frags_chain_segs_kernel, a->state,
					XFG_FRAGS_CHAIN_STATE_WORDS(a->n), ntiles, grid, s, *a);
	return err ? err : xfg_scan_launch(xfg_frags_chain_select_kernel, a->state, 0, ntiles, grid, s, *a);
}

extern "C" int xfg_launch_frags_chain_spread(const uint8_t *pv, const uint32_t *seg, uint8_t *verdicts,
					     uint32_t n, unsigned grid, void *stream)
{
	return xfg_flat_launch(xfg_frags_chain_spread_kernel, ((uint64_t)n / 4 + 255) / 256 + 1, grid,
			       stream, pv, seg, verdicts, n);
}

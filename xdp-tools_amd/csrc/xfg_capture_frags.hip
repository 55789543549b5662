// xfg_capture_frags.hip -- capture by verdict of multi-buffer AF_XDP packets:
// one pcapng Enhanced Packet Block a packet, its records' bytes concatenated
// (xfg_capture_descs_frags(), include/xdpfilter_gpu.h).  Included by
// xfg_kernels.hip in the unit with the shared kernels, after xfg_capture.hip
// whose block layout, tile shape and CP_* names it uses.
//
// Packets.  Record i is live if its verdict byte is not 0xff, and continues
// (c[i]) if it is live and has XDP_PKT_CONTD set.  A record starts a segment
// if it is not live or record i - 1 does not continue; a live segment start is
// a head.  Every live record that is no segment start follows a live record
// that continues, so its segment's start is a head and all records between
// are live: a live end-of-packet record closes the packet of its segment's
// start, and a segment that runs into a record that is not live, or into the
// end of the batch, closes nothing.
//
// Two kernels on the device's stream, both in the capture kernel's scheme
// (the tile scan of xfg_scan.hip over tiles of XFG_CAPTURE_TILE records).
//
// The scan.  A segmented forward scan over the records' lengths gives record
// i the bytes of its segment before it, off[i], and its segment's start: a
// wave scan with the start flags, an LDS step over the (pass, wave)
// aggregates {has a start, bytes since the last start (or all of them), last
// start}, and a look-back of its own (the operator is not a sum, so it is not
// xfg_lookback(); the flags and the progress argument are the same) whose
// status value is that triple in 62 bits (1 + 32 + 29; a packet is shorter
// than 2^25 bytes, and the bytes of a run that is no packet may wrap: nothing
// reads them).  The walk back ends at the first tile with a start in it,
// whether that tile has finished its own look-back or not, so a packet of
// many tiles costs a walk over its own tiles only.
// off[i] goes to library scratch; an end-of-packet record stores {off + len,
// records} into its head's slot of tot[], which the launch filled with ones:
// a slot still all ones is no head of a complete packet.  No record walks its
// packet: the cost is linear in the records whatever the packets' shapes.
//
// The copy.  xfg_capture_kernel with a packet's {bytes, records} in the place
// of a frame's length: selected heads contribute L, every other record 0; a
// lane finds its block by the search in LDS, and for a payload dword the
// record that holds its first byte by a binary search over off[] between the
// head and the packet's end (no step for a packet of one record).  The dword
// is put together from aligned 4-byte loads shifted into place: at most two
// loads a record (a record's start and the join may both be unaligned), and
// the next record that holds a byte is found by the same search, so records
// of length 0 between two joins cost a search and not a walk.  With
// XFG_CAPTURE_HEAD_ONLY the frame is the head record alone.

namespace {
constexpr int CF_SUM_BITS = 29;
constexpr unsigned long long CF_SUM = (1ull << CF_SUM_BITS) - 1;
constexpr unsigned long long CF_HAS = 1ull << 61;
constexpr unsigned long long CF_NONE = ~0ull;   // tot[]: no head of a complete packet

__device__ inline unsigned long long cf_pack(bool has, uint32_t idx, uint32_t sum)
{
	return (has ? CF_HAS : 0ull) | (unsigned long long)idx << CF_SUM_BITS | (sum & CF_SUM);
}

// The @need (1..4) bytes at offset @o of the packet whose head is record @h
// and whose records are h .. h + nrec - 1, as the low bytes of a dword.
__device__ inline uint32_t cf_payload(const xfg_capture_frags_kargs &a, uint32_t h, uint32_t nrec,
				      uint32_t o, uint32_t need)
{
	const uint64_t offp = (uint64_t)(uintptr_t)a.off, rx = (uint64_t)(uintptr_t)a.descs;
	const uint64_t fb = (uint64_t)(uintptr_t)a.umem;
	const uint32_t end = h + nrec;
	// the last record at or after lo whose off is not past the position
	uint32_t lo = h, ro = 0, got = 0, val = 0;
	for (;;) {
		for (uint32_t hi = end; hi - lo > 1u;) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			const uint32_t x = *reinterpret_cast<gu32 *>(offp + 4ull * mid);
			if (x <= o + got) {
				lo = mid;
				ro = x;
			} else {
				hi = mid;
			}
		}
		const u32x4 rec = *reinterpret_cast<gu32x4 *>(rx + 16ull * ((a.first + lo) & a.mask));
		const uint64_t addr = (uint64_t)rec.y << 32 | rec.x;
		const uint32_t b = o + got - ro;
		if (b >= rec.z)   // (only past the stated limits)
			break;
		const uint32_t take = min(rec.z - b, need - got);
		const uint64_t p = fb + (addr & XSK_ADDR) + (addr >> 48) + b;
		const uint32_t sh = (uint32_t)p & 3u;
		uint32_t w = *reinterpret_cast<gu32 *>(p - sh) >> (8u * sh);
		if (take > 4u - sh)
			w |= *reinterpret_cast<gu32 *>(p - sh + 4u) << (8u * (4u - sh));
		if (take < 4u)
			w &= (1u << (8u * take)) - 1u;
		val |= w << (8u * got);
		got += take;
		if (got >= need || ++lo >= end)
			break;
		ro = *reinterpret_cast<gu32 *>(offp + 4ull * lo);
	}
	return val;
}
}  // namespace

__global__ __launch_bounds__(CP_LANES, 4) void xfg_capture_frags_scan_kernel(
	const xfg_capture_frags_kargs a)
{
	__shared__ uint32_t s_sum[CP_PASSES * CP_WAVES], s_idx[CP_PASSES * CP_WAVES];
	__shared__ uint32_t s_has[CP_PASSES * CP_WAVES];
	__shared__ uint32_t s_csum[CP_PASSES * CP_WAVES + 1], s_cidx[CP_PASSES * CP_WAVES + 1];
	__shared__ uint32_t s_chas[CP_PASSES * CP_WAVES + 1];
	__shared__ uint32_t s_bsum, s_bidx;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_CAPTURE_TILES(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 2;
	const uint64_t rx = (uint64_t)(uintptr_t)a.descs, vd = (uint64_t)(uintptr_t)a.verdicts;
	const uint64_t offp = (uint64_t)(uintptr_t)a.off, totp = (uint64_t)(uintptr_t)a.tot;
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_CAPTURE_TILE + tid;
		uint32_t len[CP_PASSES], off[CP_PASSES], hd[CP_PASSES];
		uint32_t fl[CP_PASSES];   // 1: live, 2: continues, 4: record i - 1 continues (lane 0)
		uint32_t own = 0;   // bit k: a start at or before this lane in its wave and pass
		uint32_t eop = 0;   // bit k: a live end-of-packet record
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * CP_LANES;
			uint32_t v = 0xff;
			len[k] = 0;
			fl[k] = 0;
			if (i < n)
				v = *reinterpret_cast<gu8 *>(vd + i);
			if (v != 0xff) {
				const u32x4 rec = *reinterpret_cast<gu32x4 *>(
					rx + 16ull * ((a.first + (uint32_t)i) & a.mask));
				len[k] = rec.z;
				fl[k] = 1u | (rec.w & XSK_CONTD) << 1;
			}
			// a wave's lane 0: does record i - 1 continue?
			if (lane == 0 && i < n && i > 0 &&
			    *reinterpret_cast<gu8 *>(vd + i - 1) != 0xff)
				fl[k] |= (*reinterpret_cast<gu32 *>(
						  rx + 16ull * ((a.first + (uint32_t)i - 1u) & a.mask) + 12) &
					  XSK_CONTD) << 2;
		}
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * CP_LANES;
			const bool live = fl[k] & 1u, c = fl[k] & 2u;
			const uint32_t pc = fl[k] & 4u;
			const uint64_t bc = __ballot(c);
			const bool start = !live || !(lane ? (bc >> (lane - 1)) & 1 : pc);
			const uint64_t bs = __ballot(start);
			eop |= (uint32_t)(live && !c) << k;
			// the wave's bytes up to this record, less those before the last
			// start at or before it
			uint32_t x = len[k];
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t y = __shfl_up(x, d);
				if (lane >= d)
					x += y;
			}
			const uint64_t m = bs & (~0ull >> (63 - lane));
			const uint32_t f = m != 0, ls = f ? 63u - (uint32_t)__builtin_clzll(m) : 0u;
			const uint32_t xs = __shfl(x - len[k], (int)ls);
			if (f)
				x -= xs;
			off[k] = x - len[k];
			hd[k] = (uint32_t)(i - lane) + ls;
			own |= f << k;
			if (lane == 63) {
				s_sum[k * CP_WAVES + wave] = x;
				s_idx[k * CP_WAVES + wave] = hd[k];
				s_has[k * CP_WAVES + wave] = f;
			}
			__builtin_amdgcn_sched_barrier(0);   // (a pass at a time: its masks are scalar registers)
		}
		__syncthreads();
		// the (pass, wave) aggregates before each one, and the tile's: one
		// wave scans the 32 of them, entry g + 1 the aggregates 0 .. g
		if (wave == 0) {
			const int g = lane & 31;
			uint32_t x = s_sum[g], id = s_idx[g], f = s_has[g];
#pragma unroll
			for (int d = 1; d < 32; d <<= 1) {
				const uint32_t y = __shfl_up(x, d), yi = __shfl_up(id, d);
				const uint32_t yf = __shfl_up(f, d);
				if (lane >= d && !f) {
					x += y;
					id = yi;
					f = yf;
				}
			}
			if (lane < 32) {
				s_csum[lane + 1] = x;
				s_cidx[lane + 1] = id;
				s_chas[lane + 1] = f;
			}
			if (lane == 32)
				s_csum[0] = s_cidx[0] = s_chas[0] = 0;
		}
		__syncthreads();
		// decoupled look-back (one lane): publish the aggregate, walk back to
		// the first tile with a start in it
		if (tid == 0) {
			const uint32_t rsum = s_csum[CP_PASSES * CP_WAVES];
			const uint32_t ridx = s_cidx[CP_PASSES * CP_WAVES];
			const uint32_t rhas = s_chas[CP_PASSES * CP_WAVES];
			uint32_t bsum = 0, bidx = 0;
			if (t == 0) {   // (record 0 is a start)
				__hip_atomic_store(&status[0], CT_INC | cf_pack(true, ridx, rsum),
						   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			} else {
				__hip_atomic_store(&status[t], CT_AGG | cf_pack(rhas, ridx, rsum),
						   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				for (uint32_t p = t - 1;;) {
					const unsigned long long w = __hip_atomic_load(
						&status[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if ((w & CT_INC) || ((w & CT_AGG) && (w & CF_HAS))) {
						bsum += (uint32_t)(w & CF_SUM);
						bidx = (uint32_t)(w >> CF_SUM_BITS);
						break;
					}
					if (w & CT_AGG) {
						bsum += (uint32_t)(w & CF_SUM);
						p--;   // tile 0 always publishes CT_INC
						continue;
					}
					__builtin_amdgcn_s_sleep(1);   // predecessor still scanning
				}
				__hip_atomic_store(&status[t],
						   CT_INC | (rhas ? cf_pack(true, ridx, rsum)
								  : cf_pack(true, bidx, bsum + rsum)),
						   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
			s_bsum = bsum;
			s_bidx = bidx;
		}
		__syncthreads();
		const uint32_t bsum = s_bsum, bidx = s_bidx;
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * CP_LANES;
			if (i >= n)
				continue;
			uint32_t o = off[k], h = hd[k];
			if (!((own >> k) & 1)) {
				const bool in_tile = s_chas[k * CP_WAVES + wave];
				o += s_csum[k * CP_WAVES + wave] + (in_tile ? 0u : bsum);
				h = in_tile ? s_cidx[k * CP_WAVES + wave] : bidx;
			}
			*reinterpret_cast<gu32_w *>(offp + 4ull * i) = o;
			if ((eop >> k) & 1)
				*reinterpret_cast<gu64_w *>(totp + 8ull * h) =
					(unsigned long long)((uint32_t)i - h + 1u) << 32 | (o + len[k]);
		}
		__syncthreads();   // the aggregates and the ticket's word reused
	}
}

__global__ __launch_bounds__(CP_LANES, 4) void xfg_capture_frags_copy_kernel(
	const xfg_capture_frags_kargs a)
{
	__shared__ uint32_t s_tot[CP_PASSES * CP_WAVES];
	__shared__ unsigned long long s_base;
	__shared__ unsigned long long s_acc[3];
	// the tile's entries, [pass][wave][lane]: a block's start in its wave and
	// pass, the frame's bytes, the packet's records and the head's verdict
	// byte (0xff: not selected); a wave reads only what it wrote
	__shared__ uint32_t s_start[XFG_CAPTURE_TILE], s_len[XFG_CAPTURE_TILE];
	__shared__ uint32_t s_nrec[XFG_CAPTURE_TILE];
	__shared__ uint8_t s_v[XFG_CAPTURE_TILE];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n, snap = a.snaplen;
	const uint32_t ntiles = (uint32_t)XFG_CAPTURE_TILES(n);
	unsigned long long *state = a.state + XFG_CAPTURE_STATE_WORDS(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(state);
	unsigned long long *status = state + 2;
	const uint64_t rx = (uint64_t)(uintptr_t)a.descs, totp = (uint64_t)(uintptr_t)a.tot;
	const uint64_t vd = (uint64_t)(uintptr_t)a.verdicts, tsp = (uint64_t)(uintptr_t)a.ts_ns;
	const uint64_t out = (uint64_t)(uintptr_t)a.out, out_bytes = a.out_bytes;
	uint32_t acc_w = 0, acc_l = 0;   // this lane's packets: written, not written
	uint64_t acc_b = 0;              // bytes of the written ones
	if (tid < 3)
		s_acc[tid] = 0;
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_CAPTURE_TILE + tid;
		unsigned long long tw[CP_PASSES];
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * CP_LANES;
			tw[k] = CF_NONE;
			if (i < n)
				tw[k] = __builtin_nontemporal_load(
					reinterpret_cast<gu64 *>(totp + 8ull * i));
		}
		// a block's start: in its wave and pass ...
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * CP_LANES;
			uint32_t v = 0xff, len = 0, blen = 0;
			if (tw[k] != CF_NONE)   // the head of a complete packet
				v = *reinterpret_cast<gu8 *>(vd + i);
			if (v < 32 && ((a.action_mask >> v) & 1)) {
				len = (uint32_t)tw[k];
				if (a.head_only)
					len = (*reinterpret_cast<gu32x4 *>(
						       rx + 16ull * ((a.first + (uint32_t)i) & a.mask))).z;
				const uint32_t cap = snap && len > snap ? snap : len;
				blen = 52u + ((cap + 3u) & ~3u);
			} else {
				v = 0xff;
			}
			uint32_t x = blen;
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t y = __shfl_up(x, d);
				if (lane >= d)
					x += y;
			}
			s_start[k * CP_LANES + tid] = x - blen;
			s_len[k * CP_LANES + tid] = len;
			s_nrec[k * CP_LANES + tid] = a.head_only ? 1u : (uint32_t)(tw[k] >> 32);
			s_v[k * CP_LANES + tid] = (uint8_t)v;
			if (lane == 63)
				s_tot[k * CP_WAVES + wave] = x;
		}
		__syncthreads();
		// ... and the tile's bytes
		uint64_t agg = 0;
#pragma unroll
		for (int g = 0; g < CP_PASSES * CP_WAVES; g++)
			agg += s_tot[g];
		if (tid == 0)
			s_base = xfg_lookback<false>(status, t, agg);
		__syncthreads();
		const uint64_t base = s_base;
		uint64_t gb = base;   // the span of this wave and pass starts here
#pragma unroll 1
		for (int k = 0; k < CP_PASSES; k++) {
			for (int w = 0; w < wave; w++)
				gb += s_tot[k * CP_WAVES + w];
			const uint32_t span = s_tot[k * CP_WAVES + wave];
			const uint32_t e0 = k * CP_LANES + wave * 64;   // the wave's entries
			// this lane's own packet, for the counts
			if (s_v[e0 + lane] < 32u) {
				const uint32_t l = s_len[e0 + lane];
				const uint32_t c = snap && l > snap ? snap : l;
				const uint32_t L = 52u + ((c + 3u) & ~3u);
				if (gb + s_start[e0 + lane] + L <= out_bytes) {
					acc_w++;
					acc_b += L;
				} else {
					acc_l++;
				}
			}
			// (only what can hold a whole block is walked)
			const uint64_t room = out_bytes > gb ? out_bytes - gb : 0;
			const uint32_t limit = room < span ? (uint32_t)room : span;
			for (uint32_t p = 4u * lane; p < limit; p += 256u) {
				uint32_t j = 0, sj = 0;
#pragma unroll
				for (uint32_t step = 32; step; step >>= 1) {
					const uint32_t s = s_start[e0 + j + step];
					if (s <= p) {
						j += step;
						sj = s;
					}
				}
				const uint32_t l = s_len[e0 + j];
				const uint32_t c = snap && l > snap ? snap : l;
				const uint32_t nq = (c + 3u) >> 2, L = 52u + 4u * nq;
				if (gb + sj + L > out_bytes)
					continue;   // this block and all after it do not fit
				const uint32_t q = (p - sj) >> 2;
				// the head record of entry j (inside the batch: below 2^32)
				const uint32_t h = (uint32_t)((uint64_t)t * XFG_CAPTURE_TILE + e0 + j);
				uint32_t val = 0;
				if (q < 7u) {
					if (q == 0)
						val = 6u;
					else if (q == 1)
						val = L;
					else if (q == 3 || q == 4) {
						val = q == 3 ? (uint32_t)(a.ts0 >> 32) : (uint32_t)a.ts0;
						if (tsp)
							val = *reinterpret_cast<gu32 *>(tsp + 8ull * h +
											   (q == 3 ? 4 : 0));
					} else if (q == 5)
						val = c;
					else if (q == 6)
						val = l;
				} else if (q < 7u + nq) {
					const uint32_t o = 4u * (q - 7u);
					val = cf_payload(a, h, s_nrec[e0 + j], o, min(4u, c - o));
				} else {
					const uint32_t o = q - 7u - nq;
					if (o == 0)
						val = 0x00090007u;
					else if (o == 1)
						val = 2u | (uint32_t)s_v[e0 + j] << 8;
					else if (o == 5)
						val = L;
				}
				*reinterpret_cast<gu32_w *>(out + gb + p) = val;
			}
			for (int w = wave; w < CP_WAVES; w++)
				gb += s_tot[k * CP_WAVES + w];
		}
		__syncthreads();   // s_tot, the entries and the ticket's word reused
	}
	if (acc_w)
		atomicAdd(&s_acc[0], (unsigned long long)acc_w);
	if (acc_b)
		atomicAdd(&s_acc[1], (unsigned long long)acc_b);
	if (acc_l)
		atomicAdd(&s_acc[2], (unsigned long long)acc_l);
	__syncthreads();
	if (tid < 3 && s_acc[tid])
		atomicAdd(&a.counts[tid], s_acc[tid]);
}

extern "C" int xfg_launch_capture_frags(const struct xfg_capture_frags_kargs *a, unsigned grid,
					void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const uint64_t ntiles = XFG_CAPTURE_TILES(a->n);
	if (hipMemsetAsync(a->counts, 0, 24, s) != hipSuccess ||
	    hipMemsetAsync(a->tot, 0xff, 8ull * a->n, s) != hipSuccess)
		return -5;
	// (both kernels' state words zeroed ahead of the first)
	const int err = xfg_scan_launch(xfg_capture_frags_scan_kernel, a->state,
					XFG_CAPTURE_FRAGS_STATE_WORDS(a->n), ntiles, grid, s, *a);
	return err ? err : xfg_scan_launch(xfg_capture_frags_copy_kernel, a->state, 0, ntiles, grid, s, *a);
}

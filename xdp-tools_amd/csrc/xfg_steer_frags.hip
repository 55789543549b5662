// xfg_steer_frags.hip -- steered egress of multi-buffer packets: every live
// record of a packet follows its head record's queue
// (xfg_steer_frags_egress(), include/xdpfilter_gpu.h).  Included by
// xfg_kernels.hip behind xfg_steer.hip, whose pieces it uses: st_key(),
// st_same_queue(), the tile shape, the K-column look-back.
//
// The K-way order-preserving partition of xfg_steer.hip over "effective
// queues".  A record is live (verdict byte != XFG_VERDICT_NONE), an end of
// packet (XDP_PKT_CONTD clear), a head (live, and record 0 or behind a record
// that is not live or is an end of packet).  A head's effective queue is its
// frame's queue if its byte is PASS, STF_FILL otherwise; a record that is not
// live has STF_DEAD; a live record that is no head takes its head's -- the
// nearest head at or before it, every record between them being live.  Only
// PASS heads load a frame window, count a refusal, swap their MACs.
//
//   In the wave.  `open` = live and not an end of packet; a record is a head
//   iff it is live and the record before it is not open.  The ballot of `open`
//   gives a lane its predecessor's bit (lane 0: one 5-byte read of record
//   i - 1), the ballot of `head` its nearest head lane at or below it, and the
//   head's effective queue comes by a cross-lane read (ds_bpermute).
//
//   In the tile.  Lane 63 of a (pass, wave) slot leaves s_carry[slot]: its
//   effective queue if the slot holds a head, STF_NOHEAD if it holds none (the
//   slot then lies inside one packet, or behind its end there is nothing
//   live).  Behind one barrier every wave resolves the 32 entries for itself
//   -- a last-value scan over 32 lanes, five steps -- and a lane with no head
//   at or below it in its slot takes the last slot before it that held one,
//   or the tile's carry-in.
//
//   Across tiles.  The look-back is not widened.  A tile whose first record is
//   live behind an open record finds that packet's head itself: wave 0 walks
//   back over verdict bytes and descriptors, 64 records a step, ballots the
//   head condition, takes the nearest head, and for a PASS head loads its
//   window and runs st_key().  It waits for no workgroup, so the progress
//   argument of xfg_steer.hip stands: a tile's waits are for status words of
//   lower tiles only, and each of those is published without a wait of its
//   publisher.  The walk ends: record t*T - 1 is live and open, so it is a
//   head or record t*T - 2 is live and open, and so on down to record 0, a
//   head if live; a guard returns STF_DEAD at record 0 all the same.  Its cost
//   is the straddling packet's records before the tile, nothing else.  The
//   head's tile may be swapping the frame's MACs meanwhile: st_key() reads
//   bytes 12 and up, which the swap rewrites with their own values.
//
//   The fill side.  With records that are not live, "i minus the TX records
//   before i" is no longer the fill position; the records that are not live
//   are one more running sum.  It is known from the verdict bytes alone, so
//   it gets a column of its own behind the K columns (one word a tile,
//   XFG_STEER_FRAGS_DEAD()) and one lane of wave 1 walks it with
//   xfg_lookback() while wave 0 walks the K.  Its waits too are for lower
//   tiles' words of the same column, each published before its publisher
//   waits.  Fill records before the tile = t*T - TX before - not live before.
//
// With every record an end of packet and live this writes what
// xfg_steer_egress_kernel writes, byte for byte.

namespace {
constexpr uint32_t STF_FILL = XFG_STEER_NONE;   // a live record of a packet whose head is not PASS
constexpr uint32_t STF_DEAD = 0xfeu;            // not live
constexpr uint32_t STF_NOHEAD = 0xfdu;          // s_carry[]: no head in the slot
constexpr uint32_t STF_VNONE = 0xffu;           // XFG_VERDICT_NONE
static_assert(XFG_STEER_QUEUES <= STF_NOHEAD, "queue numbers below the three marks");

// record @i of the batch: its verdict byte and option bits say "live and the
// packet goes on"
__device__ __forceinline__ bool stf_open(const xfg_steer_kargs &a, uint64_t i)
{
	const uint32_t v = *reinterpret_cast<gu8 *>((uint64_t)(uintptr_t)a.verdicts + i);
	const uint32_t o = *reinterpret_cast<gu32 *>(
		(uint64_t)(uintptr_t)a.rx + 16ull * ((a.rx_first + (uint32_t)i) & a.rx_mask) + 12);
	return v != STF_VNONE && (o & XSK_CONTD);
}

// The effective queue of the packet that is open at record @end - 1 (live, not
// an end of packet), by the whole calling wave: back from @end, 64 records a
// step, to the nearest head.
__device__ __forceinline__ uint32_t stf_walk_back(const xfg_steer_kargs &a, uint64_t end,
						  const uint8_t *s_avail)
{
	const int lane = threadIdx.x & 63;
	const uint64_t rx = (uint64_t)(uintptr_t)a.rx, vd = (uint64_t)(uintptr_t)a.verdicts;
	const uint64_t umem = (uint64_t)(uintptr_t)a.umem;
	for (;;) {
		const int64_t j = (int64_t)end - 64 + lane;
		bool head = false;
		if (j >= 0) {
			const bool live = *reinterpret_cast<gu8 *>(vd + j) != STF_VNONE;
			head = live && !(j > 0 && stf_open(a, (uint64_t)j - 1));
		}
		const uint64_t hb = __ballot(head);
		if (hb == 0) {
			if (end <= 64)
				return STF_DEAD;   // (not reached: record 0 is a head if live)
			end -= 64;
			continue;
		}
		// (uniform from here: the head's record, by every lane)
		const uint64_t h = end - 64 + (63 - __builtin_clzll(hb));
		if (*reinterpret_cast<gu8 *>(vd + h) != A_PASS)
			return STF_FILL;
		const u32x4 rec = *reinterpret_cast<gdesc *>(rx + 16ull * ((a.rx_first + (uint32_t)h) & a.rx_mask));
		const uint64_t addr = (uint64_t)rec.y << 32 | rec.x;
		const uint64_t frame = umem + (addr & XSK_ADDR) + (addr >> 48);
		u32x4 c[4];
#pragma unroll
		for (int k = 0; k < 4; k++) {
			c[k] = u32x4{ 0, 0, 0, 0 };
			if (16u * k < rec.z)
				c[k] = *reinterpret_cast<st_gchunk *>(frame + 16 * k);
		}
		bool refused;
		const uint32_t key = st_key(c, rec.z, a.mode, frame, refused);
		return refused ? a.skip_queue : s_avail[key % a.navail];
	}
}
}  // namespace

__global__ __launch_bounds__(SC_LANES) void xfg_steer_frags_egress_kernel(const xfg_steer_kargs a)
{
	// [queue][slot]: the records of the slot's 64 that take the queue, ...
	__shared__ __attribute__((aligned(16))) uint8_t s_cnt[XFG_STEER_QUEUES * SC_SLOTS];
	// ... and those of the slots before it in the tile
	__shared__ __attribute__((aligned(16))) uint16_t s_pre[XFG_STEER_QUEUES * SC_SLOTS];
	__shared__ uint32_t s_fcnt[SC_SLOTS];          // fill-side records of a slot
	__shared__ uint32_t s_dcnt[SC_SLOTS];          // records of a slot that are not live
	__shared__ uint32_t s_carry[SC_SLOTS];         // the effective queue a slot hands on
	__shared__ uint32_t s_tin;                     // the one the tile is handed
	__shared__ uint32_t s_base[XFG_STEER_QUEUES];  // a queue's records before the tile
	__shared__ uint32_t s_pbase;                   // their sum: TX records before the tile
	__shared__ uint32_t s_dbase;                   // records before the tile that are not live
	__shared__ uint32_t s_skip;                    // refused heads of the tile
	__shared__ u32x4 s_ring[XFG_STEER_QUEUES];     // {tx lo, tx hi, first, mask}
	__shared__ uint8_t s_avail[XFG_STEER_AVAIL];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n, nq = a.nqueues;
	const uint32_t ntiles = (uint32_t)XFG_STEER_TILES(n);
	const uint32_t nbits = nq > 1 ? 32 - __builtin_clz(nq - 1) : 0;   // of a queue number
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + XFG_STEER_STATUS(0, nq);
	unsigned long long *dstatus = a.state + XFG_STEER_FRAGS_DEAD(n, nq);
	const uint64_t rx = (uint64_t)(uintptr_t)a.rx, fill = (uint64_t)(uintptr_t)a.fill;
	const uint64_t umem = (uint64_t)(uintptr_t)a.umem, vd = (uint64_t)(uintptr_t)a.verdicts;
	const uint64_t qof = (uint64_t)(uintptr_t)a.queue_of;
	if (tid < (int)nq)
		s_ring[tid] = *reinterpret_cast<st_gchunk *>((uint64_t)(uintptr_t)&a.queues[tid]);
	if (tid < (int)a.navail)
		s_avail[tid] = *reinterpret_cast<gu8 *>((uint64_t)(uintptr_t)a.avail + tid);
	for (;;) {
		reinterpret_cast<uint64_t *>(s_cnt)[tid] = 0;
		if (tid == 0)
			s_skip = 0;
		const uint32_t t = xfg_tile_ticket(ticket);   // (a barrier: the tables, the zeros)
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_STEER_TILE + tid;
		uint32_t vb[SC_PASSES];
		u32x4 rec[SC_PASSES];
		bool popen[SC_PASSES];   // lane 0: the record before the slot is open
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			vb[k] = STF_VNONE;   // (past the batch: not live)
			if (i < n)
				vb[k] = *reinterpret_cast<gu8 *>(vd + i);
		}
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			rec[k] = u32x4{ 0, 0, 0, 0 };
			if (i < n)
				rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
					rx + 16ull * ((a.rx_first + (uint32_t)i) & a.rx_mask)));
			popen[k] = false;
			if (lane == 0 && i > 0 && i < n)
				popen[k] = stf_open(a, i - 1);
		}
		// heads, and every lane's nearest head lane at or below it (64: none)
		bool head[SC_PASSES];
		uint32_t hl[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const bool live = vb[k] != STF_VNONE;
			const uint64_t ob = __ballot(live && (rec[k].w & XSK_CONTD));
			if (lane)
				popen[k] = (ob >> (lane - 1)) & 1;
			head[k] = live && !popen[k];
			const uint64_t hb = __ballot(head[k]) & (~0ull >> (63 - lane));
			hl[k] = hb ? 63u - __builtin_clzll(hb) : 64u;
			// (uniform) the records of the slot that are not live, of the batch
			const uint64_t db = __ballot(!live && i0 + (uint64_t)k * SC_LANES < n);
			if (lane == 0)
				s_dcnt[k * SC_WAVES + wave] = __builtin_popcountll(db);
		}
		// the tile's carry-in: its first record goes on a packet of an earlier tile
		if (wave == 0) {
			const bool cont = __builtin_amdgcn_readfirstlane(popen[0] && vb[0] != STF_VNONE);
			uint32_t tin = STF_DEAD;
			if (cont)
				tin = stf_walk_back(a, (uint64_t)t * XFG_STEER_TILE, s_avail);
			if (lane == 0)
				s_tin = tin;
		}
		// the queues of the PASS heads, two passes' frames in flight
		uint32_t qu[SC_PASSES];
		uint32_t skipped = 0;
#pragma unroll
		for (int k0 = 0; k0 < SC_PASSES; k0 += 2) {
			u32x4 c[2][4];
#pragma unroll
			for (int kk = 0; kk < 2; kk++) {
				const int k = k0 + kk;
				const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
				const uint64_t frame = umem + (addr & XSK_ADDR) + (addr >> 48);
				// (with the swap chunk 0 always, as xfg_swap_macs() takes it)
				const uint32_t len = a.swap_macs && rec[k].z < 1 ? 1u : rec[k].z;
#pragma unroll
				for (int j = 0; j < 4; j++) {
					c[kk][j] = u32x4{ 0, 0, 0, 0 };
					if (head[k] && vb[k] == A_PASS && 16u * j < len)
						c[kk][j] = *reinterpret_cast<st_gchunk *>(frame + 16 * j);
				}
			}
#pragma unroll
			for (int kk = 0; kk < 2; kk++) {
				const int k = k0 + kk;
				uint32_t qh = vb[k] == STF_VNONE ? STF_DEAD : STF_FILL;
				if (head[k] && vb[k] == A_PASS) {
					const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
					const uint64_t frame = umem + (addr & XSK_ADDR) + (addr >> 48);
					bool refused;
					const uint32_t key = st_key(c[kk], rec[k].z, a.mode, frame, refused);
					qh = refused ? a.skip_queue : s_avail[key % a.navail];
					skipped += refused;
					if (a.swap_macs) {
						const u32x4 h = c[kk][0];
						*reinterpret_cast<gu32x4_w *>(frame) =
							u32x4{ (h.y >> 16) | (h.z << 16), (h.z >> 16) | (h.x << 16),
							       (h.x >> 16) | (h.y << 16), h.w };
					}
				}
				// a live record takes its head's; one with no head in its slot waits
				const uint32_t got = __shfl(qh, (int)(hl[k] & 63));
				qu[k] = vb[k] == STF_VNONE ? STF_DEAD : hl[k] < 64 ? got : STF_NOHEAD;
				if (lane == 63)
					s_carry[k * SC_WAVES + wave] = qu[k];
			}
		}
		{
			// (uniform: the wave's refused heads)
			uint32_t sk = skipped;
#pragma unroll
			for (int o = 32; o; o >>= 1)
				sk += __shfl_xor(sk, o);
			if (lane == 0 && sk)
				atomicAdd(&s_skip, sk);
		}
		__syncthreads();
		{
			// slot `lane`'s entry becomes the last one at or before it that is a
			// queue; a pass's carry-in is the entry of the slot before its own
			uint32_t cy = lane < SC_SLOTS ? s_carry[lane] : STF_NOHEAD;
#pragma unroll
			for (int o = 1; o < SC_SLOTS; o <<= 1) {
				const uint32_t up = __shfl_up(cy, o);
				if (lane >= o && cy == STF_NOHEAD)
					cy = up;
			}
			const uint32_t tin = s_tin;
#pragma unroll
			for (int k = 0; k < SC_PASSES; k++) {
				const int slot = k * SC_WAVES + wave;
				uint32_t cin = __shfl(cy, slot ? slot - 1 : 0);
				if (slot == 0 || cin == STF_NOHEAD)
					cin = tin;
				if (qu[k] == STF_NOHEAD)
					qu[k] = cin;
			}
		}
		// a record's rank among its wave's and pass's records of its queue (bits
		// 0..5 of rk[k]); fill-side records before it in its wave and pass
		uint32_t rk[SC_PASSES], before[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			const bool tx = qu[k] < XFG_STEER_QUEUES;
			const uint64_t m = st_same_queue(qu[k], tx, nbits);
			rk[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
							  __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
			if (tx && rk[k] == 0)
				s_cnt[qu[k] * SC_SLOTS + k * SC_WAVES + wave] = (uint8_t)__builtin_popcountll(m);
			xfg_wave_rank<false>(qu[k] == STF_FILL, k, before[k], s_fcnt);
			if (qof && i < n)
				*reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(qof + i) =
					(uint8_t)(tx ? qu[k] : XFG_STEER_NONE);
		}
		__syncthreads();
		const uint32_t fagg = xfg_tile_step<false>(before, s_fcnt);
		if (wave == 0) {
			// queue `lane`: its 32 slot counts to exclusive prefix sums, its total
			const u32x4 lo = *reinterpret_cast<const u32x4 *>(&s_cnt[lane * SC_SLOTS]);
			const u32x4 hi = *reinterpret_cast<const u32x4 *>(&s_cnt[lane * SC_SLOTS + 16]);
			const uint32_t cw[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
			uint32_t pw[16];
			uint32_t agg = 0;
#pragma unroll
			for (int j = 0; j < 16; j++) {
				const uint32_t two = (cw[j >> 1] >> (16 * (j & 1))) & 0xffffu;
				pw[j] = agg | (agg + (two & 0xffu)) << 16;
				agg += (two & 0xffu) + (two >> 8);
			}
			u32x4 *pre = reinterpret_cast<u32x4 *>(&s_pre[lane * SC_SLOTS]);
#pragma unroll
			for (int j = 0; j < 4; j++)
				pre[j] = u32x4{ pw[4 * j], pw[4 * j + 1], pw[4 * j + 2], pw[4 * j + 3] };
			const uint32_t base = (uint32_t)xfg_lookback_wave(status, nq, t, (uint32_t)lane, agg);
			s_base[lane] = base;   // (<= n < 2^32)
			uint32_t pbase = base;
#pragma unroll
			for (int o = 32; o; o >>= 1)
				pbase += __shfl_xor(pbase, o);
			if (lane == 0) {
				s_pbase = pbase;
				if (s_skip)
					atomicAdd(&a.counts[nq + 1], (unsigned long long)s_skip);
			}
			if (t == ntiles - 1 && (uint32_t)lane < nq)
				a.counts[lane] = (unsigned long long)base + agg;
		} else if (wave == 1) {
			// the column of the records that are not live
			uint32_t dagg = lane < SC_SLOTS ? s_dcnt[lane] : 0;
#pragma unroll
			for (int o = 32; o; o >>= 1)
				dagg += __shfl_xor(dagg, o);
			if (lane == 0)
				s_dbase = (uint32_t)xfg_lookback<false>(dstatus, t, dagg);
		}
		__syncthreads();
		// fill-side records before the tile
		const uint32_t fbase = t * XFG_STEER_TILE - s_pbase - s_dbase;
		if (tid == 0 && t == ntiles - 1)
			a.counts[nq] = (unsigned long long)fbase + fagg;
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			if (qu[k] < XFG_STEER_QUEUES) {
				const uint32_t q = qu[k];
				const u32x4 ring = s_ring[q];
				const uint32_t pos = s_base[q] + s_pre[q * SC_SLOTS + k * SC_WAVES + wave] + rk[k];
				*reinterpret_cast<gdesc_w *>(((uint64_t)ring.y << 32 | ring.x) +
							     16ull * ((ring.z + pos) & ring.w)) =
					u32x4{ rec[k].x, rec[k].y, rec[k].z, rec[k].w & XSK_CONTD };
			} else if (fill && qu[k] == STF_FILL) {
				const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
				*reinterpret_cast<gu64_w *>(
					fill + 8ull * ((a.fill_first + fbase + before[k]) & a.fill_mask)) =
					addr & XSK_ADDR;
			}
		}
		__syncthreads();   // the LDS arrays / the ticket's word reused
	}
}

extern "C" int xfg_launch_steer_frags(const struct xfg_steer_kargs *a, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	// the refused heads' count: every tile adds to it
	if (hipMemsetAsync(&a->counts[a->nqueues + 1], 0, 8, s) != hipSuccess)
		return -5;
	return xfg_scan_launch(xfg_steer_frags_egress_kernel, a->state,
			       XFG_STEER_FRAGS_STATE_WORDS(a->n, a->nqueues), XFG_STEER_TILES(a->n), grid, s, *a);
}

// xfg_forward_frags.hip -- forwarded egress of multi-buffer packets: every live
// record of a packet follows its head record's port
// (xfg_forward_frags_egress(), include/xdpfilter_gpu.h).  Included by
// xfg_kernels.hip behind xfg_forward.hip and xfg_steer_frags.hip, whose pieces
// it uses: fw_parse(), the FIB gathers two passes at a time, the ifindex hash,
// the rewrite from the chunks in registers and the packed reason counts of the
// one; the open / head ballots, the head lane's cross-lane read, s_carry[] with
// its 32-entry last-value scan and the column of the records that are not live
// of the other.
//
// A record's word is queue | reason << 8.  The queue is a port, the stack ring
// (nports), FWF_FILL (a live record of a packet whose head is not PASS),
// FWF_DEAD (not live) or, until the tile has resolved it, FWF_NOHEAD; the
// reason is the head's, XFG_QUEUE_NONE with the last three.  Only PASS heads
// load a frame window, walk the FIB, count a reason; only XFG_FWD_OK heads are
// rewritten; no byte of a continuation's chunk is read or written.
//
//   Across tiles.  xfg_steer_frags.hip finds a straddling packet's head itself
//   and parses it again.  Here that would be wrong: the head's tile decrements
//   the TTL in place, and a head that came with TTL 2 reads as TTL 1 -- "to the
//   stack, XFG_FWD_TTL" -- once it is rewritten; the bytes do not tell "was 1"
//   from "was 2 and forwarded".  So no tile reads a frame another workgroup may
//   be writing: a straddling packet's word comes from the tile that owns its
//   head, through one more status column behind the K columns and the dead
//   column (XFG_FWD_FRAGS_CARRY(), a word a tile) -- a last-value carry, not a
//   sum.  A word is flag | record word: CT_INC "final", the word of the tile's
//   last record if that record is open (live, not an end of packet), FWF_DEAD
//   otherwise; CT_AGG "transparent", the tile holds no head and its last record
//   is open, so what it hands on is what it is handed.
//
//   A tile publishes its word behind its own FIB walk, before any wait: final
//   if its last record is not open or the tile holds a head (its last record's
//   head is then the tile's last head: every record between them is live, or
//   there would be a later head), transparent otherwise -- and then final too,
//   once it has its carry-in.  A tile whose first record continues an open
//   packet (fwf_carry_in(): one lane, as the dead column is walked) goes down
//   that column from tile t - 1, past transparent words, to the first final
//   one, which is its carry-in; tile 0 is never transparent, because its first
//   record is a head or not live.
//
//   Progress (xfg_scan.hip).  Every word a tile publishes first in the carry
//   column is published without a wait of its publisher, and the walk waits
//   only for such first words of lower tiles -- it passes a transparent word,
//   it does not wait for it to turn final -- so it ends.  The dead column's
//   aggregate needs the verdict bytes alone and is published without a wait.
//   The K columns' aggregates depend on the carry-in, so they are published
//   behind that wait, which ends; the K look-back then waits for lower tiles'
//   words only, each published behind waits that end, by induction from tile 0,
//   which waits for nothing.
//
// With every record an end of packet and live this writes what
// xfg_forward_egress_kernel writes, byte for byte.

namespace {
constexpr uint32_t FWF_FILL = XFG_STEER_NONE;   // a live record of a packet whose head is not PASS
constexpr uint32_t FWF_DEAD = 0xfeu;            // not live
constexpr uint32_t FWF_NOHEAD = 0xfdu;          // s_carry[]: no head in the slot
constexpr uint32_t FWF_VNONE = 0xffu;           // XFG_VERDICT_NONE
constexpr uint32_t FWF_NOREASON = XFG_STEER_NONE << 8;   // reason_of of a record of no PASS packet
static_assert(XFG_STEER_QUEUES <= FWF_NOHEAD, "queue numbers below the three marks");

// record @i of the batch: its verdict byte and option bits say "live and the
// packet goes on"
__device__ __forceinline__ bool fwf_open(const xfg_fwd_kargs &a, uint64_t i)
{
	const uint32_t v = *reinterpret_cast<gu8 *>((uint64_t)(uintptr_t)a.verdicts + i);
	const uint32_t o = *reinterpret_cast<gu32 *>(
		(uint64_t)(uintptr_t)a.rx + 16ull * ((a.rx_first + (uint32_t)i) & a.rx_mask) + 12);
	return v != FWF_VNONE && (o & XSK_CONTD);
}

// Tile @t > 0's carry-in, by one lane: the first final word of the carry
// column below it.  Relaxed agent-scope atomics: the value travels inside the
// word.
__device__ __forceinline__ uint32_t fwf_carry_in(unsigned long long *carry, uint32_t t)
{
	for (uint32_t p = t - 1;;) {
		const unsigned long long w =
			__hip_atomic_load(&carry[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (w & CT_INC)
			return (uint32_t)(w & 0xffffu);
		if (w & CT_AGG) {
			if (p == 0)
				return FWF_DEAD | FWF_NOREASON;   // (not reached: tile 0 is never transparent)
			p--;
			continue;
		}
		__builtin_amdgcn_s_sleep(1);   // the tile below is still walking its FIB
	}
}
}  // namespace

__global__ __launch_bounds__(SC_LANES) void xfg_forward_frags_egress_kernel(const xfg_fwd_kargs a)
{
	// (the forward kernel's: [queue][slot] counts, their prefix sums, ...)
	__shared__ __attribute__((aligned(16))) uint8_t s_cnt[XFG_STEER_QUEUES * SC_SLOTS];
	__shared__ __attribute__((aligned(16))) uint16_t s_pre[XFG_STEER_QUEUES * SC_SLOTS];
	__shared__ uint32_t s_fcnt[SC_SLOTS];          // fill-side records of a slot
	__shared__ uint32_t s_dcnt[SC_SLOTS];          // records of a slot that are not live
	__shared__ uint32_t s_carry[SC_SLOTS];         // the word a slot hands on
	__shared__ uint32_t s_tin;                     // the one the tile is handed
	__shared__ uint32_t s_cont;                    // the tile's first record continues an open packet
	__shared__ uint32_t s_lastopen;                // the tile's last record is open
	__shared__ uint32_t s_base[XFG_STEER_QUEUES];
	__shared__ uint32_t s_pbase;                   // TX records before the tile
	__shared__ uint32_t s_dbase;                   // records before the tile that are not live
	__shared__ u32x4 s_ring[XFG_STEER_QUEUES];     // {tx lo, tx hi, first, mask}
	__shared__ uint2 s_hash[XFG_FWD_HASH_SLOTS];   // {ifindex, queue}
	__shared__ uint32_t s_reason[XFG_FWD_NREASONS];   // the tile's PASS packets by reason
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n, nq = a.nqueues, stack = nq - 1;
	const uint32_t ntiles = (uint32_t)XFG_STEER_TILES(n);
	const uint32_t nbits = nq > 1 ? 32 - __builtin_clz(nq - 1) : 0;   // of a queue number
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + XFG_STEER_STATUS(0, nq);
	unsigned long long *dstatus = a.state + XFG_STEER_FRAGS_DEAD(n, nq);
	unsigned long long *carry = a.state + XFG_FWD_FRAGS_CARRY(n, nq);
	const uint64_t rx = (uint64_t)(uintptr_t)a.rx, fill = (uint64_t)(uintptr_t)a.fill;
	const uint64_t umem = (uint64_t)(uintptr_t)a.umem, vd = (uint64_t)(uintptr_t)a.verdicts;
	const uint64_t qof = (uint64_t)(uintptr_t)a.queue_of, rof = (uint64_t)(uintptr_t)a.reason_of;
	const uint64_t t24 = (uint64_t)(uintptr_t)a.t24, t8 = (uint64_t)(uintptr_t)a.t8;
	const uint64_t nh = (uint64_t)(uintptr_t)a.nh;
	if (tid < (int)nq)
		s_ring[tid] = *reinterpret_cast<st_gchunk *>((uint64_t)(uintptr_t)&a.queues[tid]);
	if (tid < (int)XFG_FWD_HASH_SLOTS)
		s_hash[tid] = uint2{ *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)&a.hash[tid].ifindex),
				     *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)&a.hash[tid].queue) };
	for (;;) {
		reinterpret_cast<uint64_t *>(s_cnt)[tid] = 0;
		if (tid < (int)XFG_FWD_NREASONS)
			s_reason[tid] = 0;
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
			vb[k] = FWF_VNONE;   // (past the batch: not live)
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
				popen[k] = fwf_open(a, i - 1);
		}
		// heads, and every lane's nearest head lane at or below it (64: none)
		bool head[SC_PASSES];
		uint32_t hl[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const bool live = vb[k] != FWF_VNONE;
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
			if (k == 0 && tid == 0)
				s_cont = live && popen[0];
			if (k == SC_PASSES - 1 && tid == SC_LANES - 1)
				s_lastopen = (ob >> 63) & 1;
		}
		// the words of the PASS heads, two passes' frames and lookups in flight
		uint32_t qu[SC_PASSES];
		uint32_t rc[3] = { 0, 0, 0 };   // reason r: bits 10 * (r % 3) .. of rc[r / 3]
#pragma unroll
		for (int k0 = 0; k0 < SC_PASSES; k0 += 2) {
			u32x4 c[2][4];
#pragma unroll
			for (int kk = 0; kk < 2; kk++) {
				const int k = k0 + kk;
				const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
				const uint64_t frame = umem + (addr & XSK_ADDR) + (addr >> 48);
#pragma unroll
				for (int j = 0; j < 4; j++) {
					c[kk][j] = u32x4{ 0, 0, 0, 0 };
					if (head[k] && vb[k] == A_PASS && 16u * j < rec[k].z)
						c[kk][j] = *reinterpret_cast<st_gchunk *>(frame + 16 * j);
				}
			}
			uint32_t why[2], tags[2], dst[2], d[2][6], e[2];
#pragma unroll
			for (int kk = 0; kk < 2; kk++) {
				const int k = k0 + kk;
				const uint32_t w[16] = { c[kk][0].x, c[kk][0].y, c[kk][0].z, c[kk][0].w,
							 c[kk][1].x, c[kk][1].y, c[kk][1].z, c[kk][1].w,
							 c[kk][2].x, c[kk][2].y, c[kk][2].z, c[kk][2].w,
							 c[kk][3].x, c[kk][3].y, c[kk][3].z, c[kk][3].w };
				why[kk] = fw_parse(w, rec[k].z, tags[kk], d[kk], dst[kk]);
				if (!(head[k] && vb[k] == A_PASS))
					why[kk] = XFG_STEER_NONE;
				// the first table: one entry an address's top 24 bits
				e[kk] = 0;
				if (why[kk] == FW_LOOKUP)
					e[kk] = *reinterpret_cast<gu16 *>(t24 + 2ull * (dst[kk] >> 8));
			}
#pragma unroll
			for (int kk = 0; kk < 2; kk++)   // a group's entry, for a prefix longer than /24
				if (e[kk] & XFG_FIB_MORE)
					e[kk] = *reinterpret_cast<gu16 *>(
						t8 + 2ull * ((e[kk] & ~XFG_FIB_MORE) * XFG_FIB_GROUP + (dst[kk] & 0xffu)));
			u32x4 hop[2];
			uint32_t mac2[2];
#pragma unroll
			for (int kk = 0; kk < 2; kk++) {
				hop[kk] = u32x4{ 0, 0, 0, 0 };
				mac2[kk] = 0;
				if (e[kk]) {
					const uint64_t p = nh + 32ull * (e[kk] - 1);
					hop[kk] = *reinterpret_cast<st_gchunk *>(p);
					mac2[kk] = *reinterpret_cast<gu32 *>(p + 16);
				}
			}
#pragma unroll
			for (int kk = 0; kk < 2; kk++) {
				const int k = k0 + kk;
				uint32_t r = why[kk], q = XFG_STEER_NONE;
				if (r == FW_LOOKUP) {
					const uint32_t mtu = hop[kk].y & 0xffffu;
					if (!e[kk]) {
						r = FW_NO_ROUTE;
					} else if (hop[kk].y >> 16) {
						r = FW_NH_RET;
					} else if (mtu && st_ntohs(d[kk][1]) > mtu) {   // :59: tot_len, not a len
						r = FW_FRAG;
					} else {
						r = FW_NO_PORT;   // :113-114
						const uint32_t h = xfg_fwd_hash(hop[kk].x);
						for (uint32_t p = 0; p < XFG_FWD_HASH_SLOTS; p++) {
							const uint2 s = s_hash[(h + p) & (XFG_FWD_HASH_SLOTS - 1)];
							if (s.x == hop[kk].x) {
								q = s.y;
								r = FW_OK;
							}
							if (s.x == hop[kk].x || !s.x)
								break;
						}
					}
				}
				if (r == FW_OK) {
					const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
					const uint64_t frame = umem + (addr & XSK_ADDR) + (addr >> 48);
					// ip_decrease_ttl(), :23-30: htons(0x0100) is 1 as the LE load sees it
					uint32_t check = (d[kk][3] & 0xffffu) + 1u;
					check = (check + (check >= 0xffffu)) & 0xffffu;
					const uint32_t ttlw = d[kk][2] - 0x10000u, chkw = (d[kk][3] & 0xffff0000u) | check;
					const uint32_t at = 5 + tags[kk];   // the TTL's dword; the check field's is the next
					const u32x4 c1 = c[kk][1], c2 = c[kk][2];
					*reinterpret_cast<gu32x4_w *>(frame) =
						u32x4{ hop[kk].z, hop[kk].w, mac2[kk], c[kk][0].w };   // :121-122
					if (tags[kk] <= 2)
						*reinterpret_cast<gu32x4_w *>(frame + 16) =
							u32x4{ c1.x, at == 5 ? ttlw : c1.y,
							       at == 6 ? ttlw : at == 5 ? chkw : c1.z,
							       at == 7 ? ttlw : at == 6 ? chkw : c1.w };
					if (tags[kk] >= 2)
						*reinterpret_cast<gu32x4_w *>(frame + 32) =
							u32x4{ at == 8 ? ttlw : at == 7 ? chkw : c2.x,
							       at == 9 ? ttlw : at == 8 ? chkw : c2.y,
							       at == 9 ? chkw : c2.z, c2.w };
				}
				// the head's word: of a PASS head its queue and reason
				uint32_t qh = (vb[k] == FWF_VNONE ? FWF_DEAD : FWF_FILL) | FWF_NOREASON;
				if (head[k] && vb[k] == A_PASS) {
					qh = (r == FW_OK ? q : stack) | r << 8;
					const uint32_t one = 1u << (10 * (r % 3));
					rc[0] += r < 3 ? one : 0;
					rc[1] += r >= 3 && r < 6 ? one : 0;
					rc[2] += r >= 6 ? one : 0;
				}
				// a live record takes its head's; one with no head in its slot waits
				const uint32_t got = __shfl(qh, (int)(hl[k] & 63));
				qu[k] = vb[k] == FWF_VNONE ? FWF_DEAD | FWF_NOREASON
				      : hl[k] < 64       ? got
							 : FWF_NOHEAD | FWF_NOREASON;
				if (lane == 63)
					s_carry[k * SC_WAVES + wave] = qu[k];
			}
		}
#pragma unroll
		for (int j = 0; j < 3; j++) {
			// (uniform: the wave's PASS packets of three reasons)
#pragma unroll
			for (int o = 32; o; o >>= 1)
				rc[j] += __shfl_xor(rc[j], o);
			if (lane < 3 && ((rc[j] >> (10 * lane)) & 0x3ffu))
				atomicAdd(&s_reason[3 * j + lane], (rc[j] >> (10 * lane)) & 0x3ffu);
		}
		__syncthreads();
		// slot `lane`'s entry becomes the last one at or before it that is a
		// queue; a pass's carry-in is the entry of the slot before its own
		uint32_t cy = lane < SC_SLOTS ? s_carry[lane] : FWF_NOHEAD | FWF_NOREASON;
#pragma unroll
		for (int o = 1; o < SC_SLOTS; o <<= 1) {
			const uint32_t up = __shfl_up(cy, o);
			if (lane >= o && (cy & 0xffu) == FWF_NOHEAD)
				cy = up;
		}
		if (wave == 0) {
			// the carry column: the tile's word out before its word in
			const uint32_t last = __shfl(cy, SC_SLOTS - 1);
			if (lane == 0) {
				const bool transparent = s_lastopen && (last & 0xffu) == FWF_NOHEAD;
				const unsigned long long out = s_lastopen ? last : FWF_DEAD | FWF_NOREASON;
				__hip_atomic_store(&carry[t], transparent ? CT_AGG : CT_INC | out, __ATOMIC_RELAXED,
						   __HIP_MEMORY_SCOPE_AGENT);
				uint32_t tin = FWF_DEAD | FWF_NOREASON;
				if (s_cont)
					tin = fwf_carry_in(carry, t);
				if (transparent)
					__hip_atomic_store(&carry[t], CT_INC | (unsigned long long)tin, __ATOMIC_RELAXED,
							   __HIP_MEMORY_SCOPE_AGENT);
				s_tin = tin;
			}
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
		{
			const uint32_t tin = s_tin;
#pragma unroll
			for (int k = 0; k < SC_PASSES; k++) {
				const int slot = k * SC_WAVES + wave;
				uint32_t cin = __shfl(cy, slot ? slot - 1 : 0);
				if (slot == 0 || (cin & 0xffu) == FWF_NOHEAD)
					cin = tin;
				if ((qu[k] & 0xffu) == FWF_NOHEAD)
					qu[k] = cin;
			}
		}
		// a record's rank among its wave's and pass's records of its queue (bits
		// 0..5 of rk[k]); fill-side records before it in its wave and pass
		uint32_t rk[SC_PASSES], before[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			const uint32_t q = qu[k] & 0xffu;
			const bool tx = q < XFG_STEER_QUEUES;
			const uint64_t m = st_same_queue(q, tx, nbits);
			rk[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
							  __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
			if (tx && rk[k] == 0)
				s_cnt[q * SC_SLOTS + k * SC_WAVES + wave] = (uint8_t)__builtin_popcountll(m);
			xfg_wave_rank<false>(q == FWF_FILL, k, before[k], s_fcnt);
			if (i < n) {
				if (qof)
					*reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(qof + i) =
						(uint8_t)(tx ? q : XFG_STEER_NONE);
				if (rof)
					*reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(rof + i) =
						(uint8_t)(tx ? qu[k] >> 8 : XFG_STEER_NONE);
			}
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
			if (lane == 0)
				s_pbase = pbase;
			if (lane < (int)XFG_FWD_NREASONS && s_reason[lane])
				atomicAdd(&a.counts[nq + 1 + lane], (unsigned long long)s_reason[lane]);
			if (t == ntiles - 1 && (uint32_t)lane < nq)
				a.counts[lane] = (unsigned long long)base + agg;
		}
		__syncthreads();
		// fill-side records before the tile
		const uint32_t fbase = t * XFG_STEER_TILE - s_pbase - s_dbase;
		if (tid == 0 && t == ntiles - 1)
			a.counts[nq] = (unsigned long long)fbase + fagg;
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint32_t q = qu[k] & 0xffu;
			if (q < XFG_STEER_QUEUES) {
				const u32x4 ring = s_ring[q];
				const uint32_t pos = s_base[q] + s_pre[q * SC_SLOTS + k * SC_WAVES + wave] + rk[k];
				*reinterpret_cast<gdesc_w *>(((uint64_t)ring.y << 32 | ring.x) +
							     16ull * ((ring.z + pos) & ring.w)) =
					u32x4{ rec[k].x, rec[k].y, rec[k].z, rec[k].w & XSK_CONTD };
			} else if (fill && q == FWF_FILL) {
				const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
				*reinterpret_cast<gu64_w *>(
					fill + 8ull * ((a.fill_first + fbase + before[k]) & a.fill_mask)) =
					addr & XSK_ADDR;
			}
		}
		__syncthreads();   // the LDS arrays / the ticket's word reused
	}
}

extern "C" int xfg_launch_forward_frags(const struct xfg_fwd_kargs *a, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	// the reasons' counts: every tile adds to them
	if (hipMemsetAsync(&a->counts[a->nqueues + 1], 0, 8 * XFG_FWD_NREASONS, s) != hipSuccess)
		return -5;
	return xfg_scan_launch(xfg_forward_frags_egress_kernel, a->state,
			       XFG_FWD_FRAGS_STATE_WORDS(a->n, a->nqueues), XFG_STEER_TILES(a->n), grid, s, *a);
}

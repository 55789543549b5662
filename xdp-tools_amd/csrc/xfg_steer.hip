// xfg_steer.hip -- steered egress: the PASS frames of an RX batch spread over
// K workers' TX rings by flow (xfg_steer_egress(), include/xdpfilter_gpu.h).
// Included by xfg_kernels.hip in the unit with the shared kernels.
//
// A one-pass, order-preserving K-way partition: the k-th record in batch order
// that takes queue q goes to that queue's tx[(tx_first + k) & tx_mask], the
// j-th record that is not PASS hands its chunk to fill[(fill_first + j) &
// fill_mask].  The queue is xdp-bench redirect-cpu's choice of a CPU
// (xdp-bench/xdp_redirect_cpumap.bpf.c:506-653): parse_eth (:53-96), then the
// hash of the address pair (:469-504, SuperFastHash of xdp-bench/hash_func01.h
// over four bytes) or a port at a fixed offset (:98-188), modulo the number of
// avail entries, through the avail table (cpus_available).
//
// The tile scan (xfg_scan.hip) with K sums in the place of one, tiles of
// XFG_STEER_TILE records.
//
//   The frame.  A PASS record's frame is read in 16-byte chunks, the first
//   four that begin below len: an untagged or tagged IPv4 header and every
//   IPv6 address pair end by byte 62.  The one field past byte 63 -- the
//   destination port of a double-tagged IPv6 frame, bytes 64..65 -- is a
//   four-byte load of its own, made only where that port counts (its TCP or
//   UDP header fits, so len >= 70).  An l3 offset is 14, 18 or 22: a whole
//   number of dwords behind byte 12, so the header is brought to fixed
//   register positions with selects and every field is a constant shift.
//
//   In the wave.  Six ballots over the queue number's bits (as many as nqueues
//   needs) leave every lane the mask of the lanes of its pass with its queue:
//   its rank is the mask's bits below it, the group's count the mask's bits,
//   exact whether the 64 lanes share one queue or take 64.  The group's first
//   lane stores the count to s_cnt[queue][slot], slot = (pass, wave), a byte:
//   a plain store, no two lanes of a tile share an entry.
//
//   In the tile.  Lane q of wave 0 reads queue q's 32 counts (32 bytes), sums
//   them in registers and leaves their exclusive prefix sums in
//   s_pre[queue][slot]; its total is the tile's aggregate for queue q.
//
//   Across tiles.  xfg_lookback_wave(): tile t publishes K status words, wave
//   0 walks back, lane q down queue q's column.  Progress: a lane waits only
//   for words of tiles with lower tickets, each of them published by a
//   workgroup that drew its ticket earlier and is resident, and a tile's K
//   aggregates are published before any of its lanes waits; so the argument
//   of xfg_scan.hip's header holds column by column -- tile 0 waits for
//   nothing and publishes K inclusive sums, and by induction over the tickets
//   every column's wait ends.  The lanes walk independently, so no column
//   waits for a word another column needs.
//
// A record's TX position is base[q] + s_pre[q][slot] + its rank.  The fill
// position of record i is i minus the PASS records before it: the sum of the K
// bases plus a two-way count of the tile (xfg_wave_rank(), xfg_tile_step()).
// The last tile writes counts[0 .. nqueues]; the refused frames are a plain
// sum, added to counts[nqueues + 1] (zeroed by the launch function) by every
// tile that has some.
//
// XFG_EGRESS_SWAP_MACS: the swap of xfg_swap_macs(), stored from the first
// chunk the queue choice loaded (the ethertype, bytes 12..13, keeps its
// place).

static_assert(SC_LANES * SC_PASSES == XFG_STEER_TILE, "tile shape");
static_assert(XFG_STEER_QUEUES == 64, "a lane a queue: one wave looks back");
static_assert(XFG_STEER_AVAIL <= SC_LANES, "a lane an avail entry");
static_assert(SC_SLOTS == 32, "a queue's counts: two 16-byte LDS loads");

namespace {
typedef const __attribute__((address_space(1))) u32x4 st_gchunk;

// SuperFastHash (Paul Hsieh's; xdp-bench/hash_func01.h) of the four bytes of
// @x in memory order on a little-endian machine, from @init: one round of the
// main loop, no tail, the final avalanche.
__device__ __forceinline__ uint32_t st_hash4(uint32_t x, uint32_t init)
{
	uint32_t h = init + (x & 0xffffu);
	h = (h << 16) ^ ((x >> 16) << 11) ^ h;
	h += h >> 11;
	h ^= h << 3;
	h += h >> 5;
	h ^= h << 4;
	h += h >> 17;
	h ^= h << 25;
	h += h >> 6;
	return h;
}

// ntohs of the low half of @v
__device__ __forceinline__ uint32_t st_ntohs(uint32_t v)
{
	return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu);
}

// ethertypes as a little-endian 16-bit load of their network-order bytes
constexpr uint32_t STE_8021Q = 0x0081, STE_8021AD = 0xa888, STE_IP = 0x0008, STE_IPV6 = 0xdd86;

// What the program takes modulo cpus_count: the hash, or the port.  @c: the
// frame's first four chunks (zeros where they begin at or past @len), @frame
// its address.  @refused: parse_eth() returned false.
__device__ __forceinline__ uint32_t st_key(const u32x4 (&c)[4], uint32_t len, uint32_t mode,
					   uint64_t frame, bool &refused)
{
	const uint32_t w[16] = { c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w,
				 c[2].x, c[2].y, c[2].z, c[2].w, c[3].x, c[3].y, c[3].z, c[3].w };
	refused = true;
	if (len < 14)   // :61
		return 0;
	uint32_t ty = w[3] & 0xffffu;
	if (st_ntohs(ty) < 0x0600u)   // :67
		return 0;
	uint32_t tags = 0;
	if (ty == STE_8021Q || ty == STE_8021AD) {   // :71-80
		if (len < 18)
			return 0;
		ty = w[4] & 0xffffu;
		tags = 1;
	}
	if (ty == STE_8021Q || ty == STE_8021AD) {   // :82-91
		if (len < 22)
			return 0;
		ty = w[5] & 0xffffu;
		tags = 2;
	}
	refused = false;
	const uint32_t l3 = 14 + 4 * tags;
	// d[]: the frame from byte l3 - 2 on, so l3 byte b is byte b + 2 of d
	uint32_t d[11];
#pragma unroll
	for (int j = 0; j < 11; j++)
		d[j] = tags == 0 ? w[3 + j] : tags == 1 ? w[4 + j] : w[5 + j];
	const bool hash = mode == XFG_STEER_MODE_HASH, sport = mode == XFG_STEER_MODE_SPORT;
	if (ty == STE_IP) {
		if (l3 + 20 > len)   // :106,152,198,477
			return 0;
		const uint32_t proto = d[2] >> 24;
		if (hash) {   // :480-481
			const uint32_t sa = (d[3] >> 16) | (d[4] << 16), da = (d[4] >> 16) | (d[5] << 16);
			return st_hash4(sa + da, 15485863u + proto);
		}
		const uint32_t l4 = proto == 6 ? 20u : proto == 17 ? 8u : 0u;   // :601-610
		if (!l4 || l3 + 20 + l4 > len)   // :112,158
			return 0;
		return sport ? st_ntohs(d[5] >> 16) : st_ntohs(d[6]);
	}
	if (ty == STE_IPV6) {
		if (l3 + 40 > len)   // :129,175,210,494
			return 0;
		const uint32_t nh = d[2] & 0xffu;
		if (hash) {   // :497-501
			uint32_t sum = 0;
#pragma unroll
			for (int j = 0; j < 8; j++)
				sum += (d[2 + j] >> 16) | (d[3 + j] << 16);
			return st_hash4(sum, 15485863u + nh);
		}
		const uint32_t l4 = nh == 6 ? 20u : nh == 17 ? 8u : 0u;   // :613-623
		if (!l4 || l3 + 40 + l4 > len)   // :135,181
			return 0;
		if (sport)
			return st_ntohs(d[10] >> 16);
		// the destination port, l3 + 42: behind two tags bytes 64..65 (len >= 70)
		uint32_t dp = tags == 0 ? w[14] : w[15];
		if (tags == 2)
			dp = *reinterpret_cast<gu32 *>(frame + 64);
		return st_ntohs(dp);
	}
	return 0;   // ARP and the rest: :547-549, :625-626
}

// The lanes of this wave with @valid set and this lane's queue @q, @nbits the
// bits a queue number has.
__device__ __forceinline__ uint64_t st_same_queue(uint32_t q, bool valid, uint32_t nbits)
{
	uint64_t m = __ballot(valid);
#pragma unroll
	for (uint32_t b = 0; b < 6; b++) {
		if (b >= nbits)
			break;
		const bool bit = (q >> b) & 1;
		const uint64_t bal = __ballot(bit);
		m &= bit ? bal : ~bal;
	}
	return m;
}
}  // namespace

__global__ __launch_bounds__(SC_LANES) void xfg_steer_egress_kernel(const xfg_steer_kargs a)
{
	// [queue][slot]: the records of the slot's 64 that take the queue, ...
	__shared__ __attribute__((aligned(16))) uint8_t s_cnt[XFG_STEER_QUEUES * SC_SLOTS];
	// ... and those of the slots before it in the tile
	__shared__ __attribute__((aligned(16))) uint16_t s_pre[XFG_STEER_QUEUES * SC_SLOTS];
	__shared__ uint32_t s_pcnt[SC_SLOTS];          // PASS records of a slot
	__shared__ uint32_t s_base[XFG_STEER_QUEUES];  // a queue's records before the tile
	__shared__ uint32_t s_pbase;                   // their sum: PASS records before the tile
	__shared__ uint32_t s_skip;                    // refused frames of the tile
	__shared__ u32x4 s_ring[XFG_STEER_QUEUES];     // {tx lo, tx hi, first, mask}
	__shared__ uint8_t s_avail[XFG_STEER_AVAIL];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n, nq = a.nqueues;
	const uint32_t ntiles = (uint32_t)XFG_STEER_TILES(n);
	const uint32_t nbits = nq > 1 ? 32 - __builtin_clz(nq - 1) : 0;   // of a queue number
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + XFG_STEER_STATUS(0, nq);
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
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			vb[k] = 0;
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
		}
		// the queues of the PASS records, two passes' frames in flight
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
					if (vb[k] == A_PASS && 16u * j < len)
						c[kk][j] = *reinterpret_cast<st_gchunk *>(frame + 16 * j);
				}
			}
#pragma unroll
			for (int kk = 0; kk < 2; kk++) {
				const int k = k0 + kk;
				const uint64_t i = i0 + (uint64_t)k * SC_LANES;
				qu[k] = XFG_STEER_NONE;
				if (vb[k] == A_PASS) {
					const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
					const uint64_t frame = umem + (addr & XSK_ADDR) + (addr >> 48);
					bool refused;
					const uint32_t key = st_key(c[kk], rec[k].z, a.mode, frame, refused);
					qu[k] = refused ? a.skip_queue : s_avail[key % a.navail];
					skipped += refused;
					if (a.swap_macs) {
						const u32x4 h = c[kk][0];
						*reinterpret_cast<gu32x4_w *>(frame) =
							u32x4{ (h.y >> 16) | (h.z << 16), (h.z >> 16) | (h.x << 16),
							       (h.x >> 16) | (h.y << 16), h.w };
					}
				}
				if (qof && i < n)
					*reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(qof + i) =
						(uint8_t)qu[k];
			}
		}
		// a record's rank among its wave's and pass's records of its queue (bits
		// 0..5 of rk[k]); PASS records before it in its wave and pass
		uint32_t rk[SC_PASSES], before[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const bool pass = vb[k] == A_PASS;
			const uint64_t m = st_same_queue(qu[k], pass, nbits);
			rk[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
							  __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
			if (pass && rk[k] == 0)
				s_cnt[qu[k] * SC_SLOTS + k * SC_WAVES + wave] = (uint8_t)__builtin_popcountll(m);
			xfg_wave_rank<false>(pass, k, before[k], s_pcnt);
		}
		{
			// (uniform: the wave's refused frames)
			uint32_t sk = skipped;
#pragma unroll
			for (int o = 32; o; o >>= 1)
				sk += __shfl_xor(sk, o);
			if (lane == 0 && sk)
				atomicAdd(&s_skip, sk);
		}
		__syncthreads();
		const uint32_t pagg = xfg_tile_step<false>(before, s_pcnt);
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
			if (t == ntiles - 1) {
				if ((uint32_t)lane < nq)
					a.counts[lane] = (unsigned long long)base + agg;
				if (lane == 0)
					a.counts[nq] = (unsigned long long)n - pbase - pagg;
			}
		}
		__syncthreads();
		const uint32_t pbase = s_pbase;
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			if (i >= n)
				continue;
			if (vb[k] == A_PASS) {
				const uint32_t q = qu[k];
				const u32x4 ring = s_ring[q];
				const uint32_t pos = s_base[q] + s_pre[q * SC_SLOTS + k * SC_WAVES + wave] + rk[k];
				*reinterpret_cast<gdesc_w *>(((uint64_t)ring.y << 32 | ring.x) +
							     16ull * ((ring.z + pos) & ring.w)) =
					u32x4{ rec[k].x, rec[k].y, rec[k].z, 0 };
			} else if (fill) {
				const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
				*reinterpret_cast<gu64_w *>(
					fill + 8ull * ((a.fill_first + ((uint32_t)i - (pbase + before[k]))) &
						       a.fill_mask)) = addr & XSK_ADDR;
			}
		}
		__syncthreads();   // s_cnt, s_pre, s_pcnt / the ticket's word reused
	}
}

extern "C" int xfg_launch_steer(const struct xfg_steer_kargs *a, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	// the refused frames' count: every tile adds to it
	if (hipMemsetAsync(&a->counts[a->nqueues + 1], 0, 8, s) != hipSuccess)
		return -5;
	return xfg_scan_launch(xfg_steer_egress_kernel, a->state, XFG_STEER_STATE_WORDS(a->n, a->nqueues),
			       XFG_STEER_TILES(a->n), grid, s, *a);
}

// xfg_forward.hip -- forwarded egress: the PASS frames of an RX batch sent to
// the TX ring of the egress port a FIB lookup names, their headers rewritten
// (xfg_forward_egress(), include/xdpfilter_gpu.h).  Included by
// xfg_kernels.hip behind xfg_steer.hip, whose partition this is -- the same
// tile, ballots (st_same_queue()), s_cnt / s_pre and xfg_lookback_wave() --
// with another choice of queue: xdp-forward's xdp_fwd_flags()
// (xdp-forward/xdp_forward.bpf.c:32-127) with an xfg_fib (xfg_fib.h) in the
// place of bpf_fib_lookup and TX ring q in the place of xdp_tx_ports entry q.
// Queue nports is the stack ring: every PASS frame the program returns
// XDP_PASS for.
//
// What a tile adds to the steer kernel's:
//
//   The frame.  The steer kernel's window: the first four 16-byte chunks that
//   begin below len.  parse_ethhdr (headers/xdp/parsing_helpers.h:100-134)
//   skips up to four tags, so l3 = 14 + 4 * tags <= 30 and the fixed IPv4
//   header ends by byte 50; l3 is a whole number of dwords behind byte 12, so
//   the header comes to fixed register positions with selects.
//
//   The lookup.  A chain of dependent gathers a frame: header line -> first
//   table -> (second-level group) -> next-hop record.  The frames go two passes
//   at a time, as in the steer kernel, and every level is issued for both
//   passes before either is consumed, so a wave has two requests of a level in
//   flight and the CU's sixteen waves thirty-two.  Cache policy: the tables
//   are reused (32 MiB of first table: Infinity Cache, the hot /24s and the
//   next hops in L2), so they are plain loads; the frames are plain loads too,
//   because the line just read is the line written; the RX records, read once,
//   stay nontemporal.
//
//   ifindex -> queue.  An open-addressing hash of 128 slots in LDS, built by
//   the host with the rings' table (xfg_layout.h): at most 63 slots are taken,
//   a probe is one or two LDS reads.
//
//   The rewrite.  ip_decrease_ttl() (:23-30) and the two memcpy (:121-122),
//   stored from the chunks in registers: chunk 0 with the next hop's twelve MAC
//   bytes, and the chunk or chunks that hold the TTL (byte l3 + 8) and the
//   check field (l3 + 10): chunk 1 up to two tags, chunk 2 from two tags on.
//   No lane reads a frame twice; only forwarded frames are written.
//
//   The reasons.  Nine counts a lane in three words, ten bits a count (a wave
//   has 512 records a tile), summed over the wave by shuffles, over the tile in
//   LDS, and added to counts[] once a tile by the tiles that have some.

static_assert(XFG_FWD_HASH_SLOTS == 128 && XFG_FWD_HASH_SLOTS <= SC_LANES, "a lane a slot; xfg_fwd_hash()");
static_assert(XFG_FWD_NREASONS == 9, "three words of three counts");
static_assert(sizeof(xfg_fib_nh) == 32, "a next hop: one 16-byte load and one of 4");

namespace {
constexpr uint32_t FW_OK = 0, FW_NOT_IP = 1, FW_BAD_HDR = 2, FW_TTL = 3, FW_V6 = 4, FW_NO_ROUTE = 5,
		   FW_NH_RET = 6, FW_FRAG = 7, FW_NO_PORT = 8;
constexpr uint32_t FW_LOOKUP = 0xfeu;   // an IPv4 frame on its way through the tables
static_assert(FW_LOOKUP != XFG_STEER_NONE, "a record that is not PASS looks nothing up");

__device__ __forceinline__ bool fw_vlan(uint32_t ty)
{
	return ty == STE_8021Q || ty == STE_8021AD;   // proto_is_vlan, parsing_helpers.h:89-93
}

// The program down to the lookup.  @w: the frame's first 16 dwords (zeros
// where a chunk begins at or past @len).  Returns the reason, or FW_LOOKUP
// with the tags skipped in @tags, the header's dwords from byte l3 - 2 on in
// @d (l3 byte b is byte b + 2 of d) and the destination in host order in @dst.
__device__ __forceinline__ uint32_t fw_parse(const uint32_t (&w)[16], uint32_t len, uint32_t &tags,
					     uint32_t (&d)[6], uint32_t &dst)
{
	tags = 0;
	dst = 0;
	if (len < 14)   // parsing_helpers.h:108
		return FW_NOT_IP;
	uint32_t ty = w[3] & 0xffffu;
	bool go = true;
#pragma unroll
	for (uint32_t i = 0; i < 4; i++) {   // :119-128
		go = go && fw_vlan(ty) && 18 + 4 * i <= len;
		if (go) {
			ty = w[4 + i] & 0xffffu;
			tags = i + 1;
		}
	}
	if (ty == STE_IPV6)   // xdp_forward.bpf.c:62: no IPv6 table, so XDP_PASS (:126)
		return FW_V6;
	if (ty != STE_IP)   // :81-83
		return FW_NOT_IP;
	const uint32_t l3 = 14 + 4 * tags;
#pragma unroll
	for (int j = 0; j < 6; j++)
		d[j] = tags == 0 ? w[3 + j] : tags == 1 ? w[4 + j] : tags == 2 ? w[5 + j]
		     : tags == 3 ? w[6 + j] : w[7 + j];
	if (l3 + 20 > len)   // parsing_helpers.h:209
		return FW_BAD_HDR;
	if (l3 + 4 * ((d[0] >> 16) & 0xfu) > len)   // :212-216 (no ihl >= 5 check there)
		return FW_BAD_HDR;
	if (((d[2] >> 16) & 0xffu) <= 1)   // xdp_forward.bpf.c:51
		return FW_TTL;
	dst = __builtin_bswap32((d[4] >> 16) | (d[5] << 16));   // :61
	return FW_LOOKUP;
}
}  // namespace

__global__ __launch_bounds__(SC_LANES) void xfg_forward_egress_kernel(const xfg_fwd_kargs a)
{
	// (the steer kernel's: [queue][slot] counts, their prefix sums, ...)
	__shared__ __attribute__((aligned(16))) uint8_t s_cnt[XFG_STEER_QUEUES * SC_SLOTS];
	__shared__ __attribute__((aligned(16))) uint16_t s_pre[XFG_STEER_QUEUES * SC_SLOTS];
	__shared__ uint32_t s_pcnt[SC_SLOTS];
	__shared__ uint32_t s_base[XFG_STEER_QUEUES];
	__shared__ uint32_t s_pbase;
	__shared__ u32x4 s_ring[XFG_STEER_QUEUES];     // {tx lo, tx hi, first, mask}
	__shared__ uint2 s_hash[XFG_FWD_HASH_SLOTS];   // {ifindex, queue}
	__shared__ uint32_t s_reason[XFG_FWD_NREASONS];   // the tile's PASS frames by reason
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n, nq = a.nqueues, stack = nq - 1;
	const uint32_t ntiles = (uint32_t)XFG_STEER_TILES(n);
	const uint32_t nbits = nq > 1 ? 32 - __builtin_clz(nq - 1) : 0;   // of a queue number
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + XFG_STEER_STATUS(0, nq);
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
		// the queues of the PASS records, two passes' frames and lookups in flight
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
					if (vb[k] == A_PASS && 16u * j < rec[k].z)
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
				if (vb[k] != A_PASS)
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
				const uint64_t i = i0 + (uint64_t)k * SC_LANES;
				uint32_t r = why[kk], q = XFG_STEER_NONE;
				if (r == FW_LOOKUP) {
					const uint32_t mtu = hop[kk].y & 0xffffu;
					if (!e[kk]) {
						r = FW_NO_ROUTE;
					} else if (hop[kk].y >> 16) {
						r = FW_NH_RET;
					} else if (mtu && st_ntohs(d[kk][1]) > mtu) {   // :59
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
				qu[k] = XFG_STEER_NONE;
				if (vb[k] == A_PASS) {
					qu[k] = r == FW_OK ? q : stack;
					const uint32_t one = 1u << (10 * (r % 3));
					rc[0] += r < 3 ? one : 0;
					rc[1] += r >= 3 && r < 6 ? one : 0;
					rc[2] += r >= 6 ? one : 0;
				}
				if (i < n) {
					if (qof)
						*reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(qof + i) =
							(uint8_t)qu[k];
					if (rof)
						*reinterpret_cast<__attribute__((address_space(1))) uint8_t *>(rof + i) =
							(uint8_t)r;
				}
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
#pragma unroll
		for (int j = 0; j < 3; j++) {
			// (uniform: the wave's PASS frames of three reasons)
#pragma unroll
			for (int o = 32; o; o >>= 1)
				rc[j] += __shfl_xor(rc[j], o);
			if (lane < 3 && ((rc[j] >> (10 * lane)) & 0x3ffu))
				atomicAdd(&s_reason[3 * j + lane], (rc[j] >> (10 * lane)) & 0x3ffu);
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
			if (lane == 0)
				s_pbase = pbase;
			if (lane < (int)XFG_FWD_NREASONS && s_reason[lane])
				atomicAdd(&a.counts[nq + 1 + lane], (unsigned long long)s_reason[lane]);
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
		__syncthreads();   // s_cnt, s_pre, s_pcnt, s_reason / the ticket's word reused
	}
}

extern "C" int xfg_launch_forward(const struct xfg_fwd_kargs *a, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	// the reasons' counts: every tile adds to them
	if (hipMemsetAsync(&a->counts[a->nqueues + 1], 0, 8 * XFG_FWD_NREASONS, s) != hipSuccess)
		return -5;
	return xfg_scan_launch(xfg_forward_egress_kernel, a->state, XFG_STEER_STATE_WORDS(a->n, a->nqueues),
			       XFG_STEER_TILES(a->n), grid, s, *a);
}

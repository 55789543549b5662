// xfg_socks.hip -- many AF_XDP sockets over one UMEM in one call
// (xfg_classify_socks(), xfg_socks_egress(), include/xdpfilter_gpu.h): what
// xsk_l2fwd_all() and xsk_rx_drop_all() do with a loop over the sockets
// (lib/util/xdpsock.c:1553-1576,1269-1285), each socket's batch peeked from
// its own RX ring.  Included by xfg_kernels.hip in the unit with the shared
// kernels.
//
// The sockets' batches form one flat batch: flat record base[s] + i is socket
// s's record i, base[s] the records of the sockets before s, base[nsocks] the
// total n.  The bases (at most 1025 words) are staged in LDS; a lane finds the
// socket of flat record i by binary search for the last s with base[s] <= i.
// A run of empty sockets has equal consecutive bases, and the last of equal
// bases is the socket that holds the record, so the search keeps going right
// on equality.
//
// Gather: flat[i] = the socket's RX record, one 16-byte load and store a
// record; the classify kernels then take flat as a plain descriptor array.
//
// Egress: xfg_egress.hip's one-pass order-preserving partition, segmented by
// socket: the tile scan (xfg_scan.hip) over tiles of XFG_SOCKS_TILE flat
// records.  A record counts as PASS if its verdict is XDP_PASS and its socket
// has a TX ring; the scan gives np(i), the PASS records before flat index i.
// A record's TX rank in its socket is np(i) - np(base[s]); its fill rank is
// (i - base[s]) minus that in its socket's own fill ring, i - np(i) in the
// shared one.  What remains is np(base[s]):
//   - a socket that starts inside the tile: the tile's base plus the PASS
//     records of the tile before position base[s] - tile * T, from the waves'
//     ballots and their prefix sums kept in LDS (any position, not only the
//     lane's own);
//   - the one socket carried into the tile from an earlier one (the socket of
//     the tile's first record, if it starts before it): the tile that owns
//     base[s] publishes np(base[s]) as a {flag, value} word, one a socket, in
//     the launch's state words, and this tile waits for it.
// Every tile publishes that word for every socket whose base lies in it, empty
// ones too (the last tile also for bases equal to n, the total among them), so
// the last tile can write the counts as differences of consecutive words.
//
// Progress (xfg_scan.hip): beside the look-back a tile waits for the carry,
// a word of the tile that owns an earlier flat index, and the last tile's
// counts for words of all the others -- tiles with lower numbers all.  Every
// wait is still bounded (XFG_SOCKS_SPINS polls, far past any real one): it
// gives up with state word 1 set rather than hold the device.
//
// XFG_EGRESS_SWAP_MACS: for the records that count as PASS.
//
// Not here: multi-buffer packets (xfg_socks_frags.hip, which reuses this
// file's table, search and waits), sockets over different UMEMs.

namespace {
static_assert(SC_LANES * SC_PASSES == XFG_SOCKS_TILE, "tile shape");
constexpr unsigned long long SK_SET = 1ull << 63;   // a published np(base[s]) word

// the socket of flat record i < base[nsocks]: the last s with base[s] <= i
__device__ __forceinline__ uint32_t sk_find(const uint32_t *base, uint32_t nsocks, uint32_t i)
{
	uint32_t lo = 0, hi = nsocks;   // base[lo] <= i < base[hi]
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (base[mid] <= i)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

__device__ __forceinline__ u32x4 sk_ring(const xfg_sock_ent *ents, uint32_t s, int which)
{
	return *reinterpret_cast<gu32x4 *>((uint64_t)(uintptr_t)ents +
					   (uint64_t)s * sizeof(xfg_sock_ent) + 16u * which);
}

// a published word's value, once it is set (if it never is: 0, state word 1
// set and *ok cleared)
__device__ __forceinline__ uint32_t sk_wait(unsigned long long *word, unsigned long long *state,
					    uint32_t *ok)
{
	for (uint32_t spins = 0; spins < XFG_SOCKS_SPINS; spins++) {
		const unsigned long long w =
			__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (w & SK_SET)
			return (uint32_t)w;
		__builtin_amdgcn_s_sleep(1);
	}
	__hip_atomic_store(&state[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	*ok = 0;
	return 0;
}
}  // namespace

__global__ __launch_bounds__(256) void xfg_socks_gather_kernel(const xfg_socks_gather_kargs a)
{
	__shared__ uint32_t s_sbase[XFG_SOCKS_TABLE_MAX + 1];
	for (uint32_t s = threadIdx.x; s <= a.nsocks; s += 256)
		s_sbase[s] = *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)a.base + 4ull * s);
	__syncthreads();
	const uint64_t flat = (uint64_t)(uintptr_t)a.flat;
	const uint64_t step = (uint64_t)gridDim.x * 256;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += step) {
		const uint32_t s = sk_find(s_sbase, a.nsocks, (uint32_t)i);
		const u32x4 rx = sk_ring(a.ents, s, 0);
		const uint64_t p = (uint64_t)rx.y << 32 | rx.x;
		const u32x4 rec = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
			p + 16ull * ((rx.z + ((uint32_t)i - s_sbase[s])) & rx.w)));
		*reinterpret_cast<gu32x4_w *>(flat + 16ull * i) = rec;
	}
}

__global__ __launch_bounds__(SC_LANES) void xfg_socks_egress_kernel(const xfg_socks_kargs a)
{
	__shared__ uint32_t s_sbase[XFG_SOCKS_TABLE_MAX + 1];
	__shared__ unsigned long long s_bal[SC_SLOTS + 1];   // ([SC_SLOTS]: 0, the tile's end)
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_pre[SC_SLOTS + 1];             // s_cnt's exclusive prefix sums
	__shared__ uint32_t s_base, s_carry, s_ok;
	const int tid = threadIdx.x;
	const uint32_t n = a.n, nsocks = a.nsocks;
	const uint32_t ntiles = (uint32_t)XFG_SOCKS_TILES(n);
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 2;
	unsigned long long *pub = status + ntiles;   // nsocks + 1 words
	const uint64_t fill = (uint64_t)(uintptr_t)a.fill, umem = (uint64_t)(uintptr_t)a.umem;
	const uint64_t vd = (uint64_t)(uintptr_t)a.verdicts;
	for (uint32_t s = tid; s <= nsocks; s += SC_LANES)
		s_sbase[s] = *reinterpret_cast<gu32 *>((uint64_t)(uintptr_t)a.base + 4ull * s);
	if (tid == 0)
		s_bal[SC_SLOTS] = 0;
	for (;;) {
		// (the first ticket's barrier also: the bases are staged)
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		const uint32_t t0 = t * XFG_SOCKS_TILE;   // (< n)
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t0 + tid;
		uint32_t sock[SC_PASSES];
		u32x4 rec[SC_PASSES];
		uint32_t pass = 0;   // bit k: the record of pass k goes to its socket's TX ring
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			sock[k] = 0;
			rec[k] = u32x4{ 0, 0, 0, 0 };
			if (i < n) {
				const uint32_t s = sk_find(s_sbase, nsocks, (uint32_t)i);
				const u32x4 rx = sk_ring(a.ents, s, 0), tx = sk_ring(a.ents, s, 1);
				sock[k] = s;
				rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
					((uint64_t)rx.y << 32 | rx.x) +
					16ull * ((rx.z + ((uint32_t)i - s_sbase[s])) & rx.w)));
				// (a socket without a TX ring: its verdicts are not read)
				if ((tx.x | tx.y) && *reinterpret_cast<gu8 *>(vd + i) == A_PASS)
					pass |= 1u << k;
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
		if (a.swap_macs) {
#pragma unroll
			for (int k = 0; k < SC_PASSES; k++) {
				if ((pass >> k) & 1)
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
			if (i >= n || !ok)
				continue;
			const uint32_t s = sock[k], b = s_sbase[s];
			const uint32_t np = base + before[k];   // PASS records before flat record i
			// ... and of them, those in its own socket
			const uint32_t r = np - (b < t0 ? carry : base + xfg_tile_before(s_pre, s_bal, b - t0));
			const uint64_t addr = (uint64_t)rec[k].y << 32 | rec[k].x;
			if ((pass >> k) & 1) {
				const u32x4 tx = sk_ring(a.ents, s, 1);
				*reinterpret_cast<gdesc_w *>(((uint64_t)tx.y << 32 | tx.x) +
							     16ull * ((tx.z + r) & tx.w)) =
					u32x4{ rec[k].x, rec[k].y, rec[k].z, 0 };
			} else if (fill) {
				*reinterpret_cast<gu64_w *>(
					fill + 8ull * ((a.fill_first + ((uint32_t)i - np)) & a.fill_mask)) =
					addr & XSK_ADDR;
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
					a.counts[2 * s + 1] = n - lo;
				} else {
					const uint32_t sent = sk_wait(&pub[s + 1], a.state, &got) - lo;
					a.counts[2 * s] = sent;
					a.counts[2 * s + 1] = s_sbase[s + 1] - s_sbase[s] - sent;
				}
			}
		}
		__syncthreads();   // s_cnt / s_bal / the ticket's word reused
	}
}

extern "C" int xfg_launch_socks_gather(const struct xfg_socks_gather_kargs *a, unsigned grid,
				       void *stream)
{
	return xfg_flat_launch(xfg_socks_gather_kernel, ((uint64_t)a->n + 255) / 256, grid, stream, *a);
}

extern "C" int xfg_launch_socks_egress(const struct xfg_socks_kargs *a, unsigned grid, void *stream)
{
	return xfg_scan_launch(xfg_socks_egress_kernel, a->state, XFG_SOCKS_STATE_WORDS(a->n, a->nsocks),
			       XFG_SOCKS_TILES(a->n), grid, static_cast<hipStream_t>(stream), *a);
}

// xfg_capture.hip -- capture by verdict: the selected frames of a device batch
// as finished pcapng Enhanced Packet Blocks in one contiguous device buffer
// (xfg_capture(), xfg_capture_descs(), include/xdpfilter_gpu.h).  Included by
// xfg_kernels.hip in the unit with the shared kernels.
//
// What xdpdump records at a program's exit (xdp-dump/xdpdump.c:502, the block
// of lib/util/xpcapng.c:392-479): frame i is selected if its verdict byte v is
// below 32 and bit v of action_mask is set; it is cut to cap = snaplen ?
// min(len, snaplen) : len bytes and becomes a block of L = 52 + cap4 bytes
// (cap4 = cap rounded up to 4), the bytes xfg_pcapng_write_captured() writes
// (xfg_io.c):
//
//   dword 0..6        6, L, 0, ts >> 32, (u32)ts, cap, len
//   dword 7..         cap frame bytes, zero-padded to cap4
//   then              0x00090007 (option 7, length 9), 2 | v << 8, 0, 0
//   then              0 (end of options), L
//
// One pass in the tile scan's scheme (xfg_scan.hip), over bytes instead of a
// predicate, tiles of XFG_CAPTURE_TILE packets: a wave scan over the L of the
// selected frames gives a block's start in its wave and pass, an LDS step
// over the (pass, wave) sums its start in the tile, and the look-back over
// the earlier tiles' {flag, bytes} status words (62 bits of value) the tile's
// start in the buffer.
//
// The copy is driven from the output side.  The blocks of a wave's 64 frames
// of one pass are contiguous in the buffer, so the tile's {start, len, source,
// verdict} entries go to LDS (16 bytes a packet, so no lane holds them across
// the look-back) and a wave's lanes walk that span a dword
// each, 256 contiguous bytes a step: every store instruction is one coalesced
// run whatever the frame sizes.  A lane finds its block by a 6-step binary
// search for the last entry whose start is not past its position (a frame
// that is not selected has L = 0 and shares its start with the next one, so
// the last of equal starts is the selected one), then produces its dword: a
// header field, a payload dword, the option or the trailer.  A payload dword
// is one aligned 4-byte load (frame starts are 16-byte aligned and readable
// to the next 16-byte boundary past their end); the last one is masked so the
// pad bytes are zero.  The search reads 4-byte entries: in a 32-lane half the
// 128 bytes it covers touch at most four blocks, and of 64 entries only j and
// j + 32 share a bank, so a step is at worst a 2-way conflict, and none when
// neighbouring frames are selected; lanes in one block broadcast.
//
// A block is written only if it ends at or before out_bytes.  Starts only
// grow, so the written blocks are a prefix of the selected frames.  Every
// lane counts its own frames (written, their bytes, not written); a workgroup
// adds its three sums to counts[] once, when the tiles have run out.

namespace {
constexpr int CP_LANES = SC_LANES;
constexpr int CP_PASSES = SC_PASSES;
constexpr int CP_WAVES = SC_WAVES;
static_assert(CP_LANES * CP_PASSES == XFG_CAPTURE_TILE, "tile shape");
constexpr uint64_t CP_SRC = (1ull << 56) - 1;   // a device address; the verdict byte above it
}  // namespace

__global__ __launch_bounds__(CP_LANES, 4) void xfg_capture_kernel(const xfg_capture_kargs a)
{
	__shared__ uint32_t s_tot[CP_PASSES * CP_WAVES];
	__shared__ unsigned long long s_base;
	__shared__ unsigned long long s_acc[3];
	// the tile's entries, [pass][wave][lane]: a block's start in its wave and
	// pass, the frame's length, and its address with the verdict byte in bits
	// 56..63 (0xff: not selected); a wave reads only what it wrote
	__shared__ uint32_t s_start[XFG_CAPTURE_TILE], s_len[XFG_CAPTURE_TILE];
	__shared__ uint64_t s_src[XFG_CAPTURE_TILE];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t n = a.n, snap = a.snaplen;
	const uint32_t ntiles = (uint32_t)XFG_CAPTURE_TILES(n);
	const bool descs = a.form & XFG_CAPTURE_F_DESCS, len16 = a.form & XFG_CAPTURE_F_LENS_U16;
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 2;
	const uint64_t fb = (uint64_t)(uintptr_t)a.base, offs = (uint64_t)(uintptr_t)a.offsets;
	const uint64_t lens = (uint64_t)(uintptr_t)a.lens, rx = (uint64_t)(uintptr_t)a.descs;
	const uint64_t vd = (uint64_t)(uintptr_t)a.verdicts, tsp = (uint64_t)(uintptr_t)a.ts_ns;
	const uint64_t out = (uint64_t)(uintptr_t)a.out, out_bytes = a.out_bytes;
	uint32_t acc_w = 0, acc_l = 0;   // this lane's frames: written, not written
	uint64_t acc_b = 0;              // bytes of the written ones
	if (tid < 3)
		s_acc[tid] = 0;
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_CAPTURE_TILE + tid;
		uint32_t v[CP_PASSES], len[CP_PASSES], blen[CP_PASSES];
		uint64_t src[CP_PASSES];
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * CP_LANES;
			v[k] = 0xff;
			if (i < n)
				v[k] = *reinterpret_cast<gu8 *>(vd + i);
		}
		// length and source of the selected frames only; L, 0 for the others
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * CP_LANES;
			len[k] = 0;
			src[k] = 0;
			blen[k] = 0;
			if (v[k] >= 32 || !((a.action_mask >> v[k]) & 1))
				continue;
			if (descs) {
				const u32x4 rec = *reinterpret_cast<gu32x4 *>(
					rx + 16ull * ((a.first + (uint32_t)i) & a.mask));
				const uint64_t addr = (uint64_t)rec.y << 32 | rec.x;
				src[k] = fb + (addr & XSK_ADDR) + (addr >> 48);
				len[k] = rec.z;
			} else {
				len[k] = len16 ? (uint32_t)*reinterpret_cast<gu16 *>(lens + 2 * i)
					       : *reinterpret_cast<gu32 *>(lens + 4 * i);
				src[k] = fb + (offs ? *reinterpret_cast<gu64 *>(offs + 8 * i)
						    : i * a.stride);
				// (the slot is the frame's buffer, as for the classify kernels)
				if (!offs && len[k] > a.stride)
					len[k] = a.stride;
			}
			const uint32_t cap = snap && len[k] > snap ? snap : len[k];
			blen[k] = 52u + ((cap + 3u) & ~3u);
		}
		// a block's start: in its wave and pass ...
#pragma unroll
		for (int k = 0; k < CP_PASSES; k++) {
			uint32_t x = blen[k];
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t y = __shfl_up(x, d);
				if (lane >= d)
					x += y;
			}
			s_start[k * CP_LANES + tid] = x - blen[k];
			s_len[k * CP_LANES + tid] = len[k];
			s_src[k * CP_LANES + tid] = src[k] | (uint64_t)(blen[k] ? v[k] : 0xffu) << 56;
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
			// this lane's own frame, for the counts
			if (s_src[e0 + lane] >> 56 < 32u) {
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
				uint32_t val = 0;
				if (q < 7u) {
					if (q == 0)
						val = 6u;
					else if (q == 1)
						val = L;
					else if (q == 3 || q == 4) {
						// packet of entry j, its timestamp's high or low half
						const uint64_t i = (uint64_t)t * XFG_CAPTURE_TILE + e0 + j;
						val = q == 3 ? (uint32_t)(a.ts0 >> 32) : (uint32_t)a.ts0;
						if (tsp)
							val = *reinterpret_cast<gu32 *>(tsp + 8 * i +
											   (q == 3 ? 4 : 0));
					} else if (q == 5)
						val = c;
					else if (q == 6)
						val = l;
				} else if (q < 7u + nq) {
					const uint32_t o = 4u * (q - 7u);
					val = *reinterpret_cast<gu32 *>((s_src[e0 + j] & CP_SRC) + o);
					if (o + 4u > c)   // the last dword of a cap that is no multiple of 4
						val &= (1u << (8u * (c & 3u))) - 1u;
				} else {
					const uint32_t o = q - 7u - nq;
					if (o == 0)
						val = 0x00090007u;
					else if (o == 1)
						val = 2u | (uint32_t)(s_src[e0 + j] >> 56) << 8;
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

extern "C" int xfg_launch_capture(const struct xfg_capture_kargs *a, unsigned grid, void *stream)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (hipMemsetAsync(a->counts, 0, 24, s) != hipSuccess)
		return -5;
	return xfg_scan_launch(xfg_capture_kernel, a->state, XFG_CAPTURE_STATE_WORDS(a->n),
			       XFG_CAPTURE_TILES(a->n), grid, s, *a);
}

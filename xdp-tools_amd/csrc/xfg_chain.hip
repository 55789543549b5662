// xfg_chain.hip -- chained contexts (xfg_classify_chain(),
// xfg_classify_descs_chain(), include/xdpfilter_gpu.h): the select pass over
// the verdict bytes an earlier stage wrote, and the scatter of the selected
// frames' new verdicts back into them.  Included by xfg_kernels.hip in the
// unit with the shared kernels.
//
// The dispatcher runs the next program only on the frames whose return value
// is in the previous one's chain_call_actions (lib/libxdp/xdp-dispatcher.c.in:
// 59-79).  Frame i is selected if its verdict byte v is below 32 and bit v of
// chain_mask is set (the capture kernel's rule).  The select pass is the tile
// scan (xfg_scan.hip) over tiles of XFG_CHAIN_TILE frames with that predicate:
// the exclusive prefix sum of the selected frames is the frame's place k in
// the selection, idx[k] = i, and sel[k] is the frame as a plain struct
// xdp_desc the classify kernels take -- a descriptor batch's record as
// received, a struct xfg_batch's frame as {its byte offset from data, its
// length (bounded by the slot for a fixed stride, as the classify kernels
// bound it), options 0}.  Only a selected frame's record or length is loaded.
// The last tile leaves the selected count (its inclusive sum) in state word 2.
//
// The scatter: verdicts[idx[k]] = pv[k], a lane a frame; idx ascends, so a
// wave's byte stores fall in as few lines as the selection is dense.

static_assert(SC_LANES * SC_PASSES == XFG_CHAIN_TILE, "tile shape");

__global__ __launch_bounds__(SC_LANES) void xfg_chain_select_kernel(const xfg_chain_kargs a)
{
	__shared__ uint32_t s_cnt[SC_SLOTS];
	__shared__ uint32_t s_base;
	const int tid = threadIdx.x;
	const uint32_t n = a.n;
	const uint32_t ntiles = (uint32_t)XFG_CHAIN_TILES(n);
	const bool descs = a.form & XFG_CHAIN_F_DESCS, len16 = a.form & XFG_CHAIN_F_LENS_U16;
	uint32_t *ticket = reinterpret_cast<uint32_t *>(a.state);
	unsigned long long *status = a.state + 4;
	const uint64_t rx = (uint64_t)(uintptr_t)a.descs, offs = (uint64_t)(uintptr_t)a.offsets;
	const uint64_t lens = (uint64_t)(uintptr_t)a.lens, vd = (uint64_t)(uintptr_t)a.verdicts;
	const uint64_t idx = (uint64_t)(uintptr_t)a.idx, sel = (uint64_t)(uintptr_t)a.sel;
	for (;;) {
		const uint32_t t = xfg_tile_ticket(ticket);
		if (t >= ntiles)
			break;
		// (64-bit: the last tile's lanes past the batch may pass 2^32)
		const uint64_t i0 = (uint64_t)t * XFG_CHAIN_TILE + tid;
		uint32_t v[SC_PASSES];
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			v[k] = 0xff;   // past the batch: not selected
			if (i < n)
				v[k] = *reinterpret_cast<gu8 *>(vd + i);
		}
		// the selected frames as plain descriptors
		u32x4 rec[SC_PASSES];
		uint32_t pick = 0;   // bit k: the frame of pass k is selected
#pragma unroll
		for (int k = 0; k < SC_PASSES; k++) {
			const uint64_t i = i0 + (uint64_t)k * SC_LANES;
			rec[k] = u32x4{ 0, 0, 0, 0 };
			if (v[k] >= 32 || !((a.chain_mask >> v[k]) & 1))
				continue;
			pick |= 1u << k;
			if (descs) {
				rec[k] = __builtin_nontemporal_load(reinterpret_cast<gdesc *>(
					rx + 16ull * ((a.first + (uint32_t)i) & a.mask)));
			} else {
				uint32_t len = len16 ? (uint32_t)*reinterpret_cast<gu16 *>(lens + 2 * i)
						     : *reinterpret_cast<gu32 *>(lens + 4 * i);
				const uint64_t off = offs ? *reinterpret_cast<gu64 *>(offs + 8 * i)
							  : i * a.stride;
				// (the slot is the frame's buffer, as for the classify kernels)
				if (!offs && len > a.stride)
					len = a.stride;
				rec[k] = u32x4{ (uint32_t)off, (uint32_t)(off >> 32), len, 0 };
			}
		}
		// selected frames before this lane's frame of pass k: in its wave ...
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
			if (!((pick >> k) & 1))
				continue;
			const uint32_t p = base + before[k];   // selected frames before i: <= i
			*reinterpret_cast<gu32_w *>(idx + 4ull * p) =
				(uint32_t)(i0 + (uint64_t)k * SC_LANES);
			*reinterpret_cast<gu32x4_w *>(sel + 16ull * p) = rec[k];
		}
		__syncthreads();   // s_cnt / the ticket's word reused
	}
}

__global__ __launch_bounds__(256) void xfg_chain_scatter_kernel(
	const uint8_t *__restrict__ pv, const uint32_t *__restrict__ idx,
	uint8_t *__restrict__ verdicts, uint32_t cnt)
{
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += step)
		verdicts[__builtin_nontemporal_load(idx + k)] = pv[k];
}

extern "C" int xfg_launch_chain_select(const struct xfg_chain_kargs *a, unsigned grid, void *stream)
{
	return xfg_scan_launch(xfg_chain_select_kernel, a->state, XFG_CHAIN_STATE_WORDS(a->n),
			       XFG_CHAIN_TILES(a->n), grid, static_cast<hipStream_t>(stream), *a);
}

extern "C" int xfg_launch_chain_scatter(const uint8_t *pv, const uint32_t *idx, uint8_t *verdicts,
					uint32_t cnt, unsigned grid, void *stream)
{
	return xfg_flat_launch(xfg_chain_scatter_kernel, ((uint64_t)cnt + 255) / 256, grid, stream, pv,
			       idx, verdicts, cnt);
}

/*
 * k_frame_out: one reconstructed picture in the back end's layout (NV12, luma stride = coded width W, chroma at
 * + W * H) -> the cropped frame as NV12, interleaved RGB or planar RGB at an arbitrary device address.  The
 * arithmetic is the integer conversion of include/m2dec_amd.h, bit-identical to frame_out.c.
 *
 * Purely memory-bound (1.5 W H read, 1.5 or 3 W H written), so shaped for the memory system: one lane owns a
 * 2-row x 8-column luma patch and its 4 chroma pairs — luma and chroma each fetched once, as aligned dwords (a left
 * crop of 2 mod 4 takes a third dword per row and a byte shift; the rows are dword-aligned because W is a multiple
 * of 4) — and stores whole dwords: 2 x 3 per RGB row, 2 per plane row.  Consecutive lanes own consecutive patches
 * of a row, so a wave's loads and stores cover one contiguous span per row.  The destination may have any
 * alignment (a frame of odd dword count is followed by the next one), so its stores are declared 1-byte aligned;
 * gfx950 runs global memory in unaligned access mode and keeps them dword stores.  The last patch of a row, when the
 * cropped width is no multiple of 8, goes bytewise over its valid columns only.  No LDS, no barriers.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "recon_internal.h"
#include "m2dec_amd.h"
#include "frame_out.h"

struct FrameOutArgs {
	const uint8_t *luma, *chroma;
	uint8_t *dst;
	int W;           /* source stride */
	int cl, ct;      /* left / top crop (even) */
	int cw, ch;      /* cropped size (even) */
	int npx, total;  /* patches per row, patches in all */
	int fmt;
	m2d_fo_coef_t k;
};

namespace {

struct __attribute__((packed)) U2 {
	uint32_t a, b;
};
struct __attribute__((packed)) U3 {
	uint32_t a, b, c;
};

/* source bytes [sx, sx + 8) of a dword-aligned row; mis = sx & 2 (wave-uniform: the left crop's) */
__device__ __forceinline__ void load8(const uint8_t *row, int sx, bool mis, uint32_t &lo, uint32_t &hi)
{
	const uint32_t *p = (const uint32_t *)(row + (sx & ~3));
	const uint32_t d0 = p[0], d1 = p[1];
	if (mis) { /* sx + 10 <= W here: sx + 8 <= W is even and 2 mod 4, W is 0 mod 4 */
		const uint32_t d2 = p[2];
		lo = (d0 >> 16) | (d1 << 16);
		hi = (d1 >> 16) | (d2 << 16);
	} else {
		lo = d0;
		hi = d1;
	}
}

__device__ __forceinline__ uint32_t clip255(int v) { return (uint32_t)min(max(v, 0), 255); }

__device__ __forceinline__ void rgb_of(const m2d_fo_coef_t &k, int Y, int cb, int cr, uint32_t &r, uint32_t &g, uint32_t &b)
{
	const int d = cb - 128, e = cr - 128;
	const int base = k.ky * (Y - k.yo) + 128;
	r = clip255((base + k.rv * e) >> 8);
	g = clip255((base + k.gu * d + k.gv * e) >> 8);
	b = clip255((base + k.bu * d) >> 8);
}

__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
	return a | (b << 8) | (c << 16) | (d << 24);
}

} // namespace

__global__ __launch_bounds__(256) void k_frame_out(FrameOutArgs a)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= a.total) return;
	const int py = t / a.npx, px = t - py * a.npx;
	const int x0 = px * 8, y0 = py * 2; /* y0 + 2 <= ch: ch is even */
	const int sx = x0 + a.cl, sy = y0 + a.ct;
	const size_t cw = (size_t)a.cw, plane = cw * (size_t)a.ch;
	const uint8_t *l0 = a.luma + (size_t)sy * a.W;
	const uint8_t *cr = a.chroma + (size_t)(sy >> 1) * a.W;
	const int n = a.cw - x0; /* valid columns of this patch (even, >= 2) */

	if (n < 8) {
		/* the partial last patch of a row: bytes, its valid columns only */
		for (int r = 0; r < 2; ++r) {
			const uint8_t *l = l0 + (size_t)r * a.W + sx;
			const size_t o = (size_t)(y0 + r) * cw + x0;
			for (int i = 0; i < n; ++i) {
				if (a.fmt == M2DEC_AMD_OUT_NV12) {
					a.dst[o + i] = l[i];
					if (!r) a.dst[plane + (size_t)py * cw + x0 + i] = cr[sx + i];
				} else {
					uint32_t R, G, B;
					rgb_of(a.k, l[i], cr[sx + (i & ~1)], cr[sx + (i | 1)], R, G, B);
					if (a.fmt == M2DEC_AMD_OUT_RGB) {
						uint8_t *p = a.dst + (o + i) * 3;
						p[0] = (uint8_t)R;
						p[1] = (uint8_t)G;
						p[2] = (uint8_t)B;
					} else {
						a.dst[o + i] = (uint8_t)R;
						a.dst[plane + o + i] = (uint8_t)G;
						a.dst[2 * plane + o + i] = (uint8_t)B;
					}
				}
			}
		}
		return;
	}

	const bool mis = (a.cl & 2) != 0;
	uint32_t yw[2][2], cwd[2];
	load8(l0, sx, mis, yw[0][0], yw[0][1]);
	load8(l0 + a.W, sx, mis, yw[1][0], yw[1][1]);
	load8(cr, sx, mis, cwd[0], cwd[1]);

	if (a.fmt == M2DEC_AMD_OUT_NV12) {
		*(U2 *)(a.dst + (size_t)y0 * cw + x0) = U2{yw[0][0], yw[0][1]};
		*(U2 *)(a.dst + (size_t)(y0 + 1) * cw + x0) = U2{yw[1][0], yw[1][1]};
		*(U2 *)(a.dst + plane + (size_t)py * cw + x0) = U2{cwd[0], cwd[1]};
		return;
	}
#pragma unroll
	for (int r = 0; r < 2; ++r) {
		uint32_t R[8], G[8], B[8];
#pragma unroll
		for (int i = 0; i < 8; ++i) {
			const int Y = (int)((yw[r][i >> 2] >> (8 * (i & 3))) & 255);
			const uint32_t c = cwd[i >> 2] >> (16 * ((i >> 1) & 1));
			rgb_of(a.k, Y, (int)(c & 255), (int)((c >> 8) & 255), R[i], G[i], B[i]);
		}
		const size_t o = (size_t)(y0 + r) * cw + x0;
		if (a.fmt == M2DEC_AMD_OUT_RGB) {
			uint8_t *p = a.dst + o * 3;
			*(U3 *)p = U3{pack4(R[0], G[0], B[0], R[1]), pack4(G[1], B[1], R[2], G[2]), pack4(B[2], R[3], G[3], B[3])};
			*(U3 *)(p + 12) = U3{pack4(R[4], G[4], B[4], R[5]), pack4(G[5], B[5], R[6], G[6]), pack4(B[6], R[7], G[7], B[7])};
		} else {
			*(U2 *)(a.dst + o) = U2{pack4(R[0], R[1], R[2], R[3]), pack4(R[4], R[5], R[6], R[7])};
			*(U2 *)(a.dst + plane + o) = U2{pack4(G[0], G[1], G[2], G[3]), pack4(G[4], G[5], G[6], G[7])};
			*(U2 *)(a.dst + 2 * plane + o) = U2{pack4(B[0], B[1], B[2], B[3]), pack4(B[4], B[5], B[6], B[7])};
		}
	}
}

/*
 * k_frame_scale: the scaled / normalised output of include/m2dec_amd.h — the conversion at the cropped size, the
 * horizontal then the vertical pass over host-built tap tables, the element type — bit-identical to frame_out.c.
 *
 * A 256-thread workgroup owns a 32 x 8 tile of output pixels, all three channels.  The tile's taps (its rows of the
 * two tables) go to LDS once.  It then walks the tile's source-row footprint in chunks of `rows` rows (a power of
 * two, 2 .. 16, even-aligned so that a row pair shares its chroma row): per chunk a lane takes a 2-row x 8-column
 * patch of the footprint the way k_frame_out does (aligned dwords, the funnel shift for a left crop of 2 mod 4, the
 * partial last patch of a row bytewise), converts it and leaves R | G << 8 | B << 16 per pixel in LDS; the
 * horizontal pass turns each (row, output column) into three uint16 in LDS, lanes running over the rows first so
 * that the odd row pitch spreads them over the banks; the vertical pass adds each lane's own output pixel in
 * registers.  The finished tile is laid out in LDS as the destination's bytes and leaves as dwords, one contiguous
 * segment per row (RGB) or per row and plane (RGBP), declared 1-byte aligned as in k_frame_out, the last 1 - 3
 * bytes of a segment bytewise.  Every source pixel of the footprint is fetched once per tile; the patch columns are
 * those of the cropped row, so no read leaves its dwords, and no write leaves the output frame.  Two
 * __syncthreads per chunk and two around the tile; no atomics, no loops that wait on another workgroup.
 *
 * LDS: 4224 pixels x 4 B of chunk (rows x pitch <= 4224, pitch = the widest footprint in patches x 8, + 1: the
 * 32-tap worst case, 1024 columns plus alignment, still gives 4 rows) + 3456 B of horizontal results + 2048 + 512 B
 * of weights + 160 B of starts and counts = 23072 B.
 */
#define FS_TW 32
#define FS_TH 8
#define FS_NPIX 4224
#define FS_HP 18 /* uint16 pitch of one (channel, column)'s rows: 16 rows + 2, an odd dword count */
#define FS_MT M2DEC_AMD_SCALE_MAX_TAPS

struct FrameScaleArgs {
	const uint8_t *luma, *chroma;
	uint8_t *dst;
	const int16_t *xs, *xc, *ys, *yc;
	const uint16_t *xw, *yw;
	int W;
	int cl, ct, cw, ch;
	int ow, oh;
	int pitch, rows_log2;
	int planar, dtype;
	float na[3], nb[3];
	m2d_fo_coef_t k;
};

namespace {
struct __attribute__((packed)) U1 {
	uint32_t a;
};
} // namespace

__global__ __launch_bounds__(256) void k_frame_scale(FrameScaleArgs a)
{
	__shared__ uint32_t s_rgb[FS_NPIX];
	__shared__ uint16_t s_h[3 * FS_TW * FS_HP];
	__shared__ uint16_t s_xw[FS_TW * FS_MT], s_yw[FS_TH * FS_MT];
	__shared__ int16_t s_xs[FS_TW], s_xc[FS_TW], s_ys[FS_TH], s_yc[FS_TH];
	const int tid = threadIdx.x;
	const int ox0 = blockIdx.x * FS_TW, oy0 = blockIdx.y * FS_TH;
	const int tw = min(FS_TW, a.ow - ox0), th = min(FS_TH, a.oh - oy0); /* >= 1: the grid covers ow x oh */

	for (int i = tid; i < FS_TW * FS_MT; i += 256) {
		const int o = i / FS_MT;
		s_xw[i] = o < tw ? a.xw[(size_t)(ox0 + o) * FS_MT + (i % FS_MT)] : (uint16_t)0;
	}
	{
		const int o = tid / FS_MT; /* FS_TH * FS_MT == 256 */
		s_yw[tid] = o < th ? a.yw[(size_t)(oy0 + o) * FS_MT + (tid % FS_MT)] : (uint16_t)0;
	}
	if (tid < FS_TW) {
		s_xs[tid] = tid < tw ? a.xs[ox0 + tid] : (int16_t)0;
		s_xc[tid] = tid < tw ? a.xc[ox0 + tid] : (int16_t)0;
	} else if (tid >= 64 && tid < 64 + FS_TH) {
		const int o = tid - 64;
		s_ys[o] = o < th ? a.ys[oy0 + o] : (int16_t)0;
		s_yc[o] = o < th ? a.yc[oy0 + o] : (int16_t)0;
	}
	__syncthreads();

	/* the tile's source footprint (starts and ends rise with the output index); the same in every lane */
	const int x_lo = __builtin_amdgcn_readfirstlane((int)s_xs[0]);
	const int x_hi = __builtin_amdgcn_readfirstlane((int)s_xs[tw - 1] + (int)s_xc[tw - 1]);
	const int y_lo = __builtin_amdgcn_readfirstlane((int)s_ys[0]) & ~1;
	const int y_hi = __builtin_amdgcn_readfirstlane((int)s_ys[th - 1] + (int)s_yc[th - 1]);
	const int px0 = x_lo & ~7, npatch = (x_hi - px0 + 7) >> 3;
	const int pitch = a.pitch, rl = a.rows_log2, R = 1 << rl;
	/* tables that do not belong to this geometry: nothing is read or written (the launcher built both) */
	if (x_lo < 0 || y_lo < 0 || x_hi > a.cw || y_hi > a.ch || x_hi <= x_lo || npatch * 8 >= pitch || R * pitch > FS_NPIX)
		return;

	const int ox = tid & (FS_TW - 1), oy = tid / FS_TW;
	const bool live = ox < tw && oy < th;
	const int vs = live ? (int)s_ys[oy] : 0, vn = live ? (int)s_yc[oy] : 0;
	const bool mis = (a.cl & 2) != 0;
	uint32_t acc[3] = {1u << 21, 1u << 21, 1u << 21};

	for (int cy = y_lo; cy < y_hi; cy += R) {
		const int rc = min(R, y_hi - cy), rcp = (rc + 1) >> 1; /* rows of this chunk, row pairs (2 rcp <= R) */
		for (int i = tid; i < rcp * npatch; i += 256) {
			const int rp = i / npatch, j = i - rp * npatch;
			const int x0 = px0 + 8 * j, y0 = cy + 2 * rp; /* x0 < x_hi <= cw, y0 + 2 <= ch: cy and ch are even */
			const int sx = x0 + a.cl, sy = y0 + a.ct;
			const uint8_t *l0 = a.luma + (size_t)sy * a.W;
			const uint8_t *cr = a.chroma + (size_t)(sy >> 1) * a.W;
			uint32_t *d = s_rgb + 2 * rp * pitch + 8 * j;
			const int n = a.cw - x0; /* valid columns of this patch (even, >= 2) */
			if (n < 8) { /* the partial last patch of a row: bytes, its valid columns only */
				for (int r = 0; r < 2; ++r) {
					const uint8_t *l = l0 + (size_t)r * a.W + sx;
					for (int c = 0; c < n; ++c) {
						uint32_t Rr, Gg, Bb;
						rgb_of(a.k, l[c], cr[sx + (c & ~1)], cr[sx + (c | 1)], Rr, Gg, Bb);
						d[r * pitch + c] = Rr | (Gg << 8) | (Bb << 16);
					}
				}
				continue;
			}
			uint32_t yw[2][2], cwd[2];
			load8(l0, sx, mis, yw[0][0], yw[0][1]);
			load8(l0 + a.W, sx, mis, yw[1][0], yw[1][1]);
			load8(cr, sx, mis, cwd[0], cwd[1]);
#pragma unroll
			for (int r = 0; r < 2; ++r)
#pragma unroll
				for (int c = 0; c < 8; ++c) {
					const int Y = (int)((yw[r][c >> 2] >> (8 * (c & 3))) & 255);
					const uint32_t cc = cwd[c >> 2] >> (16 * ((c >> 1) & 1));
					uint32_t Rr, Gg, Bb;
					rgb_of(a.k, Y, (int)(cc & 255), (int)((cc >> 8) & 255), Rr, Gg, Bb);
					d[r * pitch + c] = Rr | (Gg << 8) | (Bb << 16);
				}
		}
		__syncthreads();

		for (int i = tid; i < (tw << rl); i += 256) {
			const int r = i & (R - 1), o = i >> rl;
			if (r >= rc) continue;
			const int n = s_xc[o];
			const uint32_t *p = s_rgb + r * pitch + ((int)s_xs[o] - px0); /* [.., + n) inside [0, npatch * 8) */
			const uint16_t *w = s_xw + o * FS_MT;
			uint32_t hr = 32, hg = 32, hb = 32;
			for (int t = 0; t < n; ++t) {
				const uint32_t px = p[t], wt = w[t];
				hr += wt * (px & 255);
				hg += wt * ((px >> 8) & 255);
				hb += wt * (px >> 16);
			}
			s_h[(0 * FS_TW + o) * FS_HP + r] = (uint16_t)(hr >> 6);
			s_h[(1 * FS_TW + o) * FS_HP + r] = (uint16_t)(hg >> 6);
			s_h[(2 * FS_TW + o) * FS_HP + r] = (uint16_t)(hb >> 6);
		}
		__syncthreads();

		if (live) {
			const int lo = max(cy, vs), hi = min(cy + rc, vs + vn);
			for (int y = lo; y < hi; ++y) {
				const uint32_t wt = s_yw[oy * FS_MT + (y - vs)];
				acc[0] += wt * s_h[(0 * FS_TW + ox) * FS_HP + (y - cy)];
				acc[1] += wt * s_h[(1 * FS_TW + ox) * FS_HP + (y - cy)];
				acc[2] += wt * s_h[(2 * FS_TW + ox) * FS_HP + (y - cy)];
			}
		}
	}

	/* the tile as the destination's bytes, in LDS (the chunk buffer: its last reader was the horizontal pass, a
	 * barrier ago): segment `seg` is one contiguous run of the frame */
	const int es = a.dtype == M2DEC_AMD_DT_F32 ? 4 : a.dtype == M2DEC_AMD_DT_F16 ? 2 : 1;
	const int nch = a.planar ? 1 : 3;           /* channels in a segment */
	const int segcap = FS_TW * nch * es;        /* LDS bytes per segment (a multiple of 32) */
	const int seglen = tw * nch * es;           /* bytes of it that exist */
	const int nseg = a.planar ? 3 * th : th;
	uint8_t *stage = (uint8_t *)s_rgb;
	if (live) {
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const uint32_t q = min(acc[c] >> 22, 255u);
			const int off = a.planar ? (oy * 3 + c) * segcap + ox * es : oy * segcap + (ox * 3 + c) * es;
			if (a.dtype == M2DEC_AMD_DT_U8) stage[off] = (uint8_t)q;
			else {
				const float v = __fmaf_rn((float)q, a.na[c], a.nb[c]);
				if (a.dtype == M2DEC_AMD_DT_F32) s_rgb[off >> 2] = __float_as_uint(v);
				else {
					const uint16_t hb = __builtin_bit_cast(uint16_t, (_Float16)v); /* round to nearest even */
					stage[off] = (uint8_t)hb;
					stage[off + 1] = (uint8_t)(hb >> 8);
				}
			}
		}
	}
	__syncthreads();

	const int ndw = seglen >> 2, tail = seglen & 3, per = ndw + (tail ? 1 : 0);
	for (int i = tid; i < nseg * per; i += 256) {
		const int seg = i / per, dw = i - seg * per;
		size_t o;
		if (a.planar) {
			const int y = seg / 3, c = seg - 3 * y;
			o = (((size_t)c * a.oh + (size_t)(oy0 + y)) * a.ow + ox0) * es;
		} else
			o = ((size_t)(oy0 + seg) * a.ow + ox0) * 3 * es;
		uint8_t *g = a.dst + o + 4 * dw;
		if (dw < ndw) *(U1 *)g = U1{s_rgb[((seg * segcap) >> 2) + dw]};
		else
			for (int t = 0; t < tail; ++t) g[t] = stage[seg * segcap + 4 * dw + t];
	}
}

static size_t fs_align16(size_t v) { return (v + 15) & ~(size_t)15; }

void m2r_frame_scale_tables_release(m2r_fo_tables_t *tab)
{
	if (!tab) return;
	if (tab->dev) (void)hipFree(tab->dev);
	free(tab->host);
	*tab = m2r_fo_tables_t();
}

int m2r_frame_scale_tables(hipStream_t s, int W, int H, const int16_t crop[4], const m2dec_amd_devout_t *cfg,
                           m2r_fo_tables_t *tab)
{
	m2d_fo_coef_t k;
	m2d_fo_scale_t sc;
	int cw, ch;
	if (m2d_frame_out_coefs(cfg, &k) < 0 || m2d_frame_out_geometry(W, H, crop, &cw, &ch) < 0) return -1;
	if (m2d_frame_out_scale(cfg, cw, ch, &sc) < 0) return -1;
	if (!sc.scaled) return 0;
	if (!tab) return -1;
	const int key[5] = {cw, ch, sc.ow, sc.oh, sc.filter};
	if (tab->dev && !memcmp(key, tab->key, sizeof(key))) return 0;
	if (tab->dev) { /* another geometry in one back end: the kernels reading the old tables first */
		if (hipStreamSynchronize(s) != hipSuccess) return -1;
		m2r_frame_scale_tables_release(tab);
	}
	const size_t ow = (size_t)sc.ow, oh = (size_t)sc.oh;
	size_t off[7];
	off[0] = 0;
	off[1] = off[0] + fs_align16(ow * 2);
	off[2] = off[1] + fs_align16(ow * 2);
	off[3] = off[2] + fs_align16(ow * FS_MT * 2);
	off[4] = off[3] + fs_align16(oh * 2);
	off[5] = off[4] + fs_align16(oh * 2);
	off[6] = off[5] + fs_align16(oh * FS_MT * 2);
	uint8_t *host = (uint8_t *)calloc(1, off[6]);
	if (!host) return -1;
	int16_t *xs = (int16_t *)(host + off[0]), *xc = (int16_t *)(host + off[1]);
	if (m2dec_amd_scale_taps(cw, sc.ow, sc.filter, xs, xc, (uint16_t *)(host + off[2])) < 0 ||
	    m2dec_amd_scale_taps(ch, sc.oh, sc.filter, (int16_t *)(host + off[3]), (int16_t *)(host + off[4]),
	                         (uint16_t *)(host + off[5])) < 0) {
		free(host);
		return -1;
	}
	/* the widest tile footprint in whole patches, as the kernel counts it */
	int widest = 0;
	for (int o0 = 0; o0 < sc.ow; o0 += FS_TW) {
		const int o1 = (o0 + FS_TW < sc.ow ? o0 + FS_TW : sc.ow) - 1;
		const int px0 = xs[o0] & ~7, np = (xs[o1] + xc[o1] - px0 + 7) >> 3;
		if (np * 8 > widest) widest = np * 8;
	}
	const int pitch = widest + 1; /* odd: rows fall on different banks */
	int rl = 4;
	while (rl > 0 && (pitch << rl) > FS_NPIX) --rl;
	void *dev = nullptr;
	if (rl < 1 || hipMalloc(&dev, off[6]) != hipSuccess) {
		free(host);
		return -1;
	}
	if (hipMemcpyAsync(dev, host, off[6], hipMemcpyHostToDevice, s) != hipSuccess) {
		(void)hipFree(dev);
		free(host);
		return -1;
	}
	tab->dev = dev;
	tab->host = host;
	memcpy(tab->key, key, sizeof(key));
	tab->pitch = pitch;
	tab->rows = 1 << rl;
	tab->rows_log2 = rl;
	for (int i = 0; i < 6; ++i) tab->off[i] = off[i];
	return 0;
}

/* enqueue the conversion of the picture at `pic` (W x H coded, the back end's layout) on stream s; every access
 * of the kernel lies inside pic[0, 1.5 W H) and dst[0, m2dec_amd_frame_out_bytes2) for what passes these checks */
int m2r_frame_out_launch(hipStream_t s, const uint8_t *pic, int W, int H, const int16_t crop[4],
                         const m2dec_amd_devout_t *cfg, uint8_t *dst, m2r_fo_tables_t *tab)
{
	FrameOutArgs a;
	m2d_fo_scale_t sc;
	int cw, ch;
	if (!pic || !dst || ((uintptr_t)pic & 3) || W <= 0 || H <= 0 || (W & 3) || (H & 1)) return -1;
	if (m2d_frame_out_coefs(cfg, &a.k) < 0 || m2d_frame_out_geometry(W, H, crop, &cw, &ch) < 0) return -1;
	if (m2d_frame_out_scale(cfg, cw, ch, &sc) < 0) return -1;
	if (sc.scaled) {
		FrameScaleArgs f;
		if (((uintptr_t)dst & (uintptr_t)(sc.esize - 1)) || m2r_frame_scale_tables(s, W, H, crop, cfg, tab) < 0) return -1;
		const uint8_t *t = (const uint8_t *)tab->dev;
		f.luma = pic;
		f.chroma = pic + (size_t)W * H;
		f.dst = dst;
		f.xs = (const int16_t *)(t + tab->off[0]);
		f.xc = (const int16_t *)(t + tab->off[1]);
		f.xw = (const uint16_t *)(t + tab->off[2]);
		f.ys = (const int16_t *)(t + tab->off[3]);
		f.yc = (const int16_t *)(t + tab->off[4]);
		f.yw = (const uint16_t *)(t + tab->off[5]);
		f.W = W;
		f.cl = crop[0];
		f.ct = crop[2];
		f.cw = cw;
		f.ch = ch;
		f.ow = sc.ow;
		f.oh = sc.oh;
		f.pitch = tab->pitch;
		f.rows_log2 = tab->rows_log2;
		f.planar = cfg->format == M2DEC_AMD_OUT_RGBP;
		f.dtype = sc.dtype;
		for (int c = 0; c < 3; ++c) {
			f.na[c] = sc.a[c];
			f.nb[c] = sc.b[c];
		}
		f.k = a.k;
		hipLaunchKernelGGL(k_frame_scale, dim3((unsigned)((sc.ow + FS_TW - 1) / FS_TW), (unsigned)((sc.oh + FS_TH - 1) / FS_TH)),
		                   dim3(256), 0, s, f);
		return hipGetLastError() == hipSuccess ? 0 : -1;
	}
	a.luma = pic;
	a.chroma = pic + (size_t)W * H;
	a.dst = dst;
	a.W = W;
	a.cl = crop[0];
	a.ct = crop[2];
	a.cw = cw;
	a.ch = ch;
	a.npx = (cw + 7) / 8;
	a.total = a.npx * (ch / 2);
	a.fmt = cfg->format;
	hipLaunchKernelGGL(k_frame_out, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, a);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int m2dec_amd_hip_frame_convert(int device, const uint8_t *luma, const uint8_t *chroma, int width, int height,
                                           const int16_t crop[4], const m2dec_amd_devout_t *cfg, uint8_t *out_host,
                                           size_t out_offset)
{
	const size_t guard = 64;
	m2d_fo_coef_t k;
	int cw, ch, r = -1;
	if (!luma || !chroma || !out_host || out_offset > 15 || width <= 0 || height <= 0 || (width & 3) || (height & 1)) return -1;
	if (m2d_frame_out_coefs(cfg, &k) < 0 || m2d_frame_out_geometry(width, height, crop, &cw, &ch) < 0) return -1;
	m2d_fo_scale_t sc;
	m2r_fo_tables_t tab; /* (this entry may allocate per call) */
	if (m2d_frame_out_scale(cfg, cw, ch, &sc) < 0 || out_offset % (size_t)sc.esize) return -1;
	const size_t bytes = m2dec_amd_frame_out_bytes2(cfg, cw, ch, nullptr, nullptr), ls = (size_t)width * height;
	uint8_t *pic = nullptr, *out = nullptr;
	if (!bytes || hipSetDevice(device) != hipSuccess) return -1;
	if (hipMalloc(&pic, ls * 3 / 2) == hipSuccess && hipMalloc(&out, bytes + 2 * guard + 16) == hipSuccess &&
	    hipMemset(out, 0xA5, bytes + 2 * guard + 16) == hipSuccess &&
	    hipMemcpy(pic, luma, ls, hipMemcpyHostToDevice) == hipSuccess &&
	    hipMemcpy(pic + ls, chroma, ls / 2, hipMemcpyHostToDevice) == hipSuccess &&
	    m2r_frame_out_launch(nullptr, pic, width, height, crop, cfg, out + guard + out_offset, &tab) == 0 &&
	    hipStreamSynchronize(nullptr) == hipSuccess &&
	    hipMemcpy(out_host, out + out_offset, bytes + 2 * guard, hipMemcpyDeviceToHost) == hipSuccess)
		r = 0;
	if (r < 0) fprintf(stderr, "m2dec_amd: frame_convert on device %d failed (%s)\n", device, hipGetErrorString(hipGetLastError()));
	if (tab.dev) (void)hipStreamSynchronize(nullptr);
	m2r_frame_scale_tables_release(&tab);
	(void)hipFree(pic);
	(void)hipFree(out);
	return r;
}

extern "C" void *m2dec_amd_device_alloc(int device, size_t bytes)
{
	void *p = nullptr;
	if (!bytes || hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) return nullptr;
	return p;
}

extern "C" void m2dec_amd_device_free(int device, void *p)
{
	if (p && hipSetDevice(device) == hipSuccess) (void)hipFree(p);
}

extern "C" int m2dec_amd_device_read(int device, const void *src_dev, void *dst_host, size_t bytes)
{
	if (!bytes) return 0;
	if (!src_dev || !dst_host || hipSetDevice(device) != hipSuccess) return -1;
	return hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

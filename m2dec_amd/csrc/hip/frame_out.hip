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

/* enqueue the conversion of the picture at `pic` (W x H coded, the back end's layout) on stream s; every access
 * of the kernel lies inside pic[0, 1.5 W H) and dst[0, m2dec_amd_frame_out_bytes) for what passes these checks */
int m2r_frame_out_launch(hipStream_t s, const uint8_t *pic, int W, int H, const int16_t crop[4],
                         const m2dec_amd_devout_t *cfg, uint8_t *dst)
{
	FrameOutArgs a;
	int cw, ch;
	if (!pic || !dst || ((uintptr_t)pic & 3) || W <= 0 || H <= 0 || (W & 3) || (H & 1)) return -1;
	if (m2d_frame_out_coefs(cfg, &a.k) < 0 || m2d_frame_out_geometry(W, H, crop, &cw, &ch) < 0) return -1;
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
	const size_t bytes = m2dec_amd_frame_out_bytes(cfg->format, cw, ch), ls = (size_t)width * height;
	uint8_t *pic = nullptr, *out = nullptr;
	if (!bytes || hipSetDevice(device) != hipSuccess) return -1;
	if (hipMalloc(&pic, ls * 3 / 2) == hipSuccess && hipMalloc(&out, bytes + 2 * guard + 16) == hipSuccess &&
	    hipMemset(out, 0xA5, bytes + 2 * guard + 16) == hipSuccess &&
	    hipMemcpy(pic, luma, ls, hipMemcpyHostToDevice) == hipSuccess &&
	    hipMemcpy(pic + ls, chroma, ls / 2, hipMemcpyHostToDevice) == hipSuccess &&
	    m2r_frame_out_launch(nullptr, pic, width, height, crop, cfg, out + guard + out_offset) == 0 &&
	    hipStreamSynchronize(nullptr) == hipSuccess &&
	    hipMemcpy(out_host, out + out_offset, bytes + 2 * guard, hipMemcpyDeviceToHost) == hipSuccess)
		r = 0;
	if (r < 0) fprintf(stderr, "m2dec_amd: frame_convert on device %d failed (%s)\n", device, hipGetErrorString(hipGetLastError()));
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

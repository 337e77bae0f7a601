/*
 * The output conversion of include/m2dec_amd.h ("device-resident output") over a host frame, in plain C: cropped
 * NV12, interleaved RGB or planar RGB.  It is the model the gfx950 kernel (m2dec_amd/csrc/hip/frame_out.hip,
 * k_frame_out) is compared with bit for bit, and an export of its own for callers of the CPU paths.
 * The coefficient rows are within 1 LSB of the float BT.601 / BT.709 matrices over all 2^24 (Y, Cb, Cr); the
 * terms stay within +-600 * 256, far inside int32.
 */
#include <stddef.h>
#include <string.h>
#include "m2dec_amd.h"
#include "frame_out.h"

int m2d_frame_out_coefs(const m2dec_amd_devout_t *cfg, m2d_fo_coef_t *k)
{
	static const m2d_fo_coef_t rows[2][2] = {
		/* [matrix][full_range]: ky, yo, rv, gu, gv, bu */
		{{298, 16, 459, -55, -136, 541}, {256, 0, 403, -48, -120, 475}},   /* BT.709 */
		{{298, 16, 409, -100, -208, 516}, {256, 0, 359, -88, -183, 454}}, /* BT.601 */
	};
	if (!cfg || cfg->size < offsetof(m2dec_amd_devout_t, frame_dst)) return -1;
	if (cfg->format < M2DEC_AMD_OUT_NV12 || cfg->format > M2DEC_AMD_OUT_RGBP) return -1;
	if (cfg->matrix != M2DEC_AMD_BT709 && cfg->matrix != M2DEC_AMD_BT601) return -1;
	*k = rows[cfg->matrix][cfg->full_range != 0];
	return 0;
}

int m2d_frame_out_geometry(int width, int height, const int16_t crop[4], int *cw, int *ch)
{
	if (width <= 0 || height <= 0 || !crop) return -1;
	for (int i = 0; i < 4; ++i)
		if (crop[i] < 0 || (crop[i] & 1)) return -1; /* an odd crop is refused, never rounded */
	const int w = width - crop[0] - crop[1], h = height - crop[2] - crop[3];
	if (w < 2 || h < 2 || (w & 1) || (h & 1)) return -1;
	*cw = w;
	*ch = h;
	return 0;
}

size_t m2dec_amd_frame_out_bytes(int format, int width, int height)
{
	if (width < 2 || height < 2 || ((width | height) & 1)) return 0;
	if (format == M2DEC_AMD_OUT_NV12) return (size_t)width * (size_t)height * 3 / 2;
	if (format == M2DEC_AMD_OUT_RGB || format == M2DEC_AMD_OUT_RGBP) return (size_t)width * (size_t)height * 3;
	return 0;
}

static inline uint8_t clip255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

int m2dec_amd_frame_convert_host(const m2d_frame_t *f, const m2dec_amd_devout_t *cfg, uint8_t *out)
{
	m2d_fo_coef_t k;
	int cw, ch;
	if (!f || !out || !f->luma || !f->chroma || m2d_frame_out_coefs(cfg, &k) < 0) return -1;
	if (m2d_frame_out_geometry(f->width, f->height, f->crop, &cw, &ch) < 0) return -1;
	const size_t stride = (size_t)f->width;
	const int cl = f->crop[0], ct = f->crop[2];
	if (cfg->format == M2DEC_AMD_OUT_NV12) {
		for (int y = 0; y < ch; ++y) memcpy(out + (size_t)y * cw, f->luma + (size_t)(y + ct) * stride + cl, (size_t)cw);
		out += (size_t)cw * ch;
		for (int y = 0; y < ch / 2; ++y)
			memcpy(out + (size_t)y * cw, f->chroma + (size_t)(y + ct / 2) * stride + cl, (size_t)cw);
		return 0;
	}
	const size_t plane = (size_t)cw * ch;
	for (int y = 0; y < ch; ++y) {
		const uint8_t *ly = f->luma + (size_t)(y + ct) * stride;
		const uint8_t *lc = f->chroma + (size_t)((y + ct) >> 1) * stride;
		for (int x = 0; x < cw; ++x) {
			const int sx = x + cl;
			const int c = ly[sx] - k.yo, d = lc[(sx >> 1) * 2] - 128, e = lc[(sx >> 1) * 2 + 1] - 128;
			const int base = k.ky * c + 128;
			const uint8_t r = clip255((base + k.rv * e) >> 8);
			const uint8_t g = clip255((base + k.gu * d + k.gv * e) >> 8);
			const uint8_t b = clip255((base + k.bu * d) >> 8);
			const size_t i = (size_t)y * cw + x;
			if (cfg->format == M2DEC_AMD_OUT_RGB) {
				out[3 * i] = r;
				out[3 * i + 1] = g;
				out[3 * i + 2] = b;
			} else {
				out[i] = r;
				out[plane + i] = g;
				out[2 * plane + i] = b;
			}
		}
	}
	return 0;
}

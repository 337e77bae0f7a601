/*
 * The output conversion of include/m2dec_amd.h ("device-resident output") over a host frame, in plain C: cropped
 * NV12, interleaved RGB or planar RGB.  It is the model the gfx950 kernel (m2dec_amd/csrc/hip/frame_out.hip,
 * k_frame_out) is compared with bit for bit, and an export of its own for callers of the CPU paths.
 * The coefficient rows are within 1 LSB of the float BT.601 / BT.709 matrices over all 2^24 (Y, Cb, Cr); the
 * terms stay within +-600 * 256, far inside int32.
 * The scaled / normalised form (tap tables, horizontal then vertical pass, element type) is the model of
 * k_frame_scale in the same way; its tables come from the one function the kernel's launcher uses too.
 */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
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

/* ---- the tap tables of the scaled output (include/m2dec_amd.h): 64-bit integers, one function for the host model
 * and the kernel's launcher */
#define SCALE_MAX_LEN 16384

static inline int64_t scale_rnd(int64_t c, int64_t T) { return (2 * c * M2DEC_AMD_SCALE_ONE + T) / (2 * T); }

int m2d_scale_taps_row(int S, int On, int filter, int o, int *start, uint16_t w[M2DEC_AMD_SCALE_MAX_TAPS])
{
	int idx[M2DEC_AMD_SCALE_MAX_TAPS];
	int64_t v[M2DEC_AMD_SCALE_MAX_TAPS], T;
	int n = 0;
	if (filter == M2DEC_AMD_SCALE_BILINEAR) {
		const int64_t num = (int64_t)(2 * o + 1) * S - On, den = 2 * (int64_t)On;
		const int64_t i0 = num >= 0 ? num / den : -((-num + den - 1) / den); /* floor */
		const int64_t rem = num - i0 * den;
		const int64_t raw_i[2] = {i0, i0 + 1}, raw_v[2] = {den - rem, rem};
		T = den;
		for (int k = 0; k < 2; ++k) {
			const int i = (int)(raw_i[k] < 0 ? 0 : raw_i[k] > S - 1 ? S - 1 : raw_i[k]);
			if (n && idx[n - 1] == i) v[n - 1] += raw_v[k]; /* clamped onto the same index: merged */
			else {
				idx[n] = i;
				v[n++] = raw_v[k];
			}
		}
	} else {
		const int64_t lo = (int64_t)o * S, hi = lo + S;
		const int first = (int)(lo / On), last = (int)((hi - 1) / On); /* every i with a positive overlap; last < S */
		T = S;
		if (last - first + 1 > M2DEC_AMD_SCALE_MAX_TAPS) return -1; /* (each of them keeps a weight >= 1: T <= ONE) */
		for (int i = first; i <= last; ++i) {
			const int64_t a = (int64_t)i * On, b = a + On;
			idx[n] = i;
			v[n++] = (b < hi ? b : hi) - (a > lo ? a : lo);
		}
	}
	int64_t c = 0;
	uint16_t wk[M2DEC_AMD_SCALE_MAX_TAPS];
	for (int k = 0; k < n; ++k) {
		wk[k] = (uint16_t)(scale_rnd(c + v[k], T) - scale_rnd(c, T));
		c += v[k];
	}
	int a = 0, b = n; /* weight-0 taps at either end are dropped (the weights sum to ONE: one stays) */
	while (a < b && !wk[a]) ++a;
	while (b > a && !wk[b - 1]) --b;
	*start = idx[a];
	for (int k = a; k < b; ++k) w[k - a] = wk[k];
	return b - a;
}

static int scale_args_ok(int S, int On, int filter)
{
	return S >= 1 && On >= 1 && S <= SCALE_MAX_LEN && On <= SCALE_MAX_LEN &&
	       (filter == M2DEC_AMD_SCALE_BILINEAR || filter == M2DEC_AMD_SCALE_AREA);
}

/* 0 if every output of the axis has at most MAX_TAPS taps */
static int scale_axis_ok(int S, int On, int filter)
{
	uint16_t w[M2DEC_AMD_SCALE_MAX_TAPS];
	int st;
	if (!scale_args_ok(S, On, filter)) return -1;
	for (int o = 0; o < On; ++o)
		if (m2d_scale_taps_row(S, On, filter, o, &st, w) < 0) return -1;
	return 0;
}

int m2dec_amd_scale_taps(int S, int On, int filter, int16_t *start, int16_t *count, uint16_t *weights)
{
	if (!start || !count || !weights || scale_axis_ok(S, On, filter) < 0) return -1; /* (checked before a write) */
	for (int o = 0; o < On; ++o) {
		uint16_t *w = weights + (size_t)o * M2DEC_AMD_SCALE_MAX_TAPS;
		int st;
		memset(w, 0, sizeof(uint16_t) * M2DEC_AMD_SCALE_MAX_TAPS);
		count[o] = (int16_t)m2d_scale_taps_row(S, On, filter, o, &st, w);
		start[o] = (int16_t)st;
	}
	return 0;
}

int m2d_frame_out_scale(const m2dec_amd_devout_t *cfg, int cw, int ch, m2d_fo_scale_t *s)
{
	memset(s, 0, sizeof(*s));
	s->ow = cw;
	s->oh = ch;
	s->esize = 1;
	if (!cfg || cw < 2 || ch < 2) return -1;
	if (cfg->size < offsetof(m2dec_amd_devout_t, std) + sizeof(cfg->std)) return 0; /* a revision-6 caller */
	if ((cfg->out_width != 0 || cfg->out_height != 0) && (cfg->out_width < 1 || cfg->out_height < 1)) return -1;
	if (cfg->filter != M2DEC_AMD_SCALE_BILINEAR && cfg->filter != M2DEC_AMD_SCALE_AREA) return -1;
	if (cfg->dtype != M2DEC_AMD_DT_U8 && cfg->dtype != M2DEC_AMD_DT_F16 && cfg->dtype != M2DEC_AMD_DT_F32) return -1;
	if (!cfg->out_width && cfg->dtype == M2DEC_AMD_DT_U8) return 0;
	if (cfg->format == M2DEC_AMD_OUT_NV12) return -1;
	s->scaled = 1;
	if (cfg->out_width) {
		s->ow = cfg->out_width;
		s->oh = cfg->out_height;
	}
	s->filter = cfg->filter;
	s->dtype = cfg->dtype;
	s->esize = cfg->dtype == M2DEC_AMD_DT_F32 ? 4 : cfg->dtype == M2DEC_AMD_DT_F16 ? 2 : 1;
	if (scale_axis_ok(cw, s->ow, s->filter) < 0 || scale_axis_ok(ch, s->oh, s->filter) < 0) return -1;
	if (cfg->dtype != M2DEC_AMD_DT_U8)
		for (int c = 0; c < 3; ++c) {
			const double mean = (double)cfg->mean[c], std = (double)cfg->std[c];
			if (!isfinite(mean) || !isfinite(std) || !(std > 0)) return -1;
			s->a[c] = (float)(1.0 / (255.0 * std));
			s->b[c] = (float)(-mean / std);
		}
	return 0;
}

size_t m2dec_amd_frame_out_bytes2(const m2dec_amd_devout_t *cfg, int crop_w, int crop_h, int *out_w, int *out_h)
{
	m2d_fo_coef_t k;
	m2d_fo_scale_t sc;
	if (m2d_frame_out_coefs(cfg, &k) < 0 || !m2dec_amd_frame_out_bytes(cfg->format, crop_w, crop_h)) return 0;
	if (m2d_frame_out_scale(cfg, crop_w, crop_h, &sc) < 0) return 0;
	if (out_w) *out_w = sc.ow;
	if (out_h) *out_h = sc.oh;
	if (!sc.scaled) return m2dec_amd_frame_out_bytes(cfg->format, crop_w, crop_h);
	return (size_t)sc.ow * (size_t)sc.oh * 3 * (size_t)sc.esize;
}

static inline uint8_t clip255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

/* float -> IEEE binary16 bits, round to nearest even (finite input or not) */
static uint16_t f16_bits(float f)
{
	uint32_t u;
	memcpy(&u, &f, 4);
	const uint16_t sign = (uint16_t)((u >> 16) & 0x8000);
	const uint32_t au = u & 0x7fffffffu;
	if (au >= 0x7f800000u) return (uint16_t)(sign | 0x7c00 | (au > 0x7f800000u ? 0x200 : 0)); /* inf / NaN */
	if (au >= 0x477ff000u) return (uint16_t)(sign | 0x7c00);                                   /* rounds to >= 65520: inf */
	if (au < 0x33000001u) return sign;                                                         /* <= 2^-25: 0 */
	const int e = (int)(au >> 23) - 127;
	uint32_t man = (au & 0x7fffffu) | 0x800000u;
	const int shift = e < -14 ? 13 + (-14 - e) : 13; /* subnormal halves lose more bits */
	const uint32_t half = 1u << (shift - 1), rest = man & ((1u << shift) - 1);
	man >>= shift;
	if (rest > half || (rest == half && (man & 1))) ++man;
	/* normal: man carries the hidden bit at 1 << 10, so adding the exponent field less one lets a rounding
	 * carry move into the exponent; subnormal: man is the field itself (a carry makes the smallest normal) */
	return (uint16_t)(sign | (e < -14 ? man : (((uint32_t)(e + 15 - 1) << 10) + man)));
}

/* the scaled path: conversion at cw x ch, horizontal pass into uint16, vertical pass, element type */
static int convert_scaled(const m2d_frame_t *f, const m2dec_amd_devout_t *cfg, const m2d_fo_coef_t *k,
                          const m2d_fo_scale_t *sc, int cw, int ch, uint8_t *out)
{
	const int ow = sc->ow, oh = sc->oh, MT = M2DEC_AMD_SCALE_MAX_TAPS;
	const size_t stride = (size_t)f->width, plane = (size_t)cw * ch, oplane = (size_t)ow * oh;
	const int cl = f->crop[0], ct = f->crop[2];
	uint8_t *rgb = (uint8_t *)malloc(3 * plane);
	uint16_t *hp = (uint16_t *)malloc(sizeof(uint16_t) * 3 * (size_t)ch * ow);
	int16_t *tab = (int16_t *)malloc(sizeof(int16_t) * (size_t)(ow + oh) * (2 + MT));
	int r = -1;
	if (rgb && hp && tab) {
		int16_t *xs = tab, *xc = xs + ow, *ys = xc + ow, *yc = ys + oh;
		uint16_t *xw = (uint16_t *)(yc + oh), *yw = xw + (size_t)ow * MT;
		if (m2dec_amd_scale_taps(cw, ow, sc->filter, xs, xc, xw) == 0 && m2dec_amd_scale_taps(ch, oh, sc->filter, ys, yc, yw) == 0) {
			for (int y = 0; y < ch; ++y) {
				const uint8_t *ly = f->luma + (size_t)(y + ct) * stride;
				const uint8_t *lc = f->chroma + (size_t)((y + ct) >> 1) * stride;
				for (int x = 0; x < cw; ++x) {
					const int sx = x + cl;
					const int c = ly[sx] - k->yo, d = lc[(sx >> 1) * 2] - 128, e = lc[(sx >> 1) * 2 + 1] - 128;
					const int base = k->ky * c + 128;
					const size_t i = (size_t)y * cw + x;
					rgb[i] = clip255((base + k->rv * e) >> 8);
					rgb[plane + i] = clip255((base + k->gu * d + k->gv * e) >> 8);
					rgb[2 * plane + i] = clip255((base + k->bu * d) >> 8);
				}
			}
			for (int c = 0; c < 3; ++c)
				for (int y = 0; y < ch; ++y) {
					const uint8_t *row = rgb + (size_t)c * plane + (size_t)y * cw;
					uint16_t *h = hp + ((size_t)c * ch + y) * ow;
					for (int x = 0; x < ow; ++x) {
						uint32_t a = 32;
						for (int t = 0; t < xc[x]; ++t) a += (uint32_t)xw[(size_t)x * MT + t] * row[xs[x] + t];
						h[x] = (uint16_t)(a >> 6);
					}
				}
			for (int c = 0; c < 3; ++c)
				for (int y = 0; y < oh; ++y)
					for (int x = 0; x < ow; ++x) {
						uint32_t a = 1u << 21;
						for (int t = 0; t < yc[y]; ++t)
							a += (uint32_t)yw[(size_t)y * MT + t] * hp[((size_t)c * ch + ys[y] + t) * ow + x];
						const uint32_t q = clip255((int)(a >> 22));
						const size_t i = cfg->format == M2DEC_AMD_OUT_RGB ? 3 * ((size_t)y * ow + x) + c
						                                                  : (size_t)c * oplane + (size_t)y * ow + x;
						if (sc->dtype == M2DEC_AMD_DT_U8) out[i] = (uint8_t)q;
						else {
							const float v = fmaf((float)q, sc->a[c], sc->b[c]);
							if (sc->dtype == M2DEC_AMD_DT_F32) memcpy(out + 4 * i, &v, 4);
							else {
								const uint16_t hb = f16_bits(v);
								memcpy(out + 2 * i, &hb, 2);
							}
						}
					}
			r = 0;
		}
	}
	free(rgb);
	free(hp);
	free(tab);
	return r;
}

int m2dec_amd_frame_convert_host(const m2d_frame_t *f, const m2dec_amd_devout_t *cfg, uint8_t *out)
{
	m2d_fo_coef_t k;
	m2d_fo_scale_t sc;
	int cw, ch;
	if (!f || !out || !f->luma || !f->chroma || m2d_frame_out_coefs(cfg, &k) < 0) return -1;
	if (m2d_frame_out_geometry(f->width, f->height, f->crop, &cw, &ch) < 0) return -1;
	if (m2d_frame_out_scale(cfg, cw, ch, &sc) < 0) return -1;
	if (sc.scaled) return convert_scaled(f, cfg, &k, &sc, cw, ch, out);
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

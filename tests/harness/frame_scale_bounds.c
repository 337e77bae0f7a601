/*
 * Bounds check of the scaled output's host side, stand-alone: m2dec_amd_scale_taps and
 * m2dec_amd_frame_convert_host over the test geometries (tests/_frame_scale.py), every plane, table and output
 * buffer a malloc of exactly its size.  Built by tests/test_frame_scale_cpu.py together with frame_out.c under
 * -fsanitize=address,undefined and run as a child process; prints "BOUNDS_OK <checks>" and exits 0, or exits 1
 * with the first check that failed (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "m2dec_amd.h"

static int checks;

#define CHECK(c)                                                        \
	do {                                                                \
		if (!(c)) {                                                     \
			fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
			exit(1);                                                    \
		}                                                               \
		++checks;                                                       \
	} while (0)

static void taps_case(int S, int On, int filter, int expect)
{
	int16_t *start = (int16_t *)malloc(sizeof(int16_t) * (size_t)On);
	int16_t *count = (int16_t *)malloc(sizeof(int16_t) * (size_t)On);
	uint16_t *w = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)On * M2DEC_AMD_SCALE_MAX_TAPS);
	CHECK(start && count && w);
	memset(start, 0x5a, sizeof(int16_t) * (size_t)On);
	CHECK(m2dec_amd_scale_taps(S, On, filter, start, count, w) == expect);
	if (expect == 0)
		for (int o = 0; o < On; ++o) {
			long sum = 0;
			CHECK(count[o] >= 1 && count[o] <= M2DEC_AMD_SCALE_MAX_TAPS && start[o] >= 0 && start[o] + count[o] <= S);
			for (int t = 0; t < M2DEC_AMD_SCALE_MAX_TAPS; ++t) {
				sum += w[(size_t)o * M2DEC_AMD_SCALE_MAX_TAPS + t];
				CHECK(t < count[o] || !w[(size_t)o * M2DEC_AMD_SCALE_MAX_TAPS + t]);
			}
			CHECK(sum == M2DEC_AMD_SCALE_ONE);
		}
	else
		CHECK(start[0] == 0x5a5a); /* refused: nothing written */
	free(start);
	free(count);
	free(w);
}

static void convert_case(int w, int h, const int16_t crop[4], int ow, int oh)
{
	const size_t ls = (size_t)w * h;
	uint8_t *luma = (uint8_t *)malloc(ls), *chroma = (uint8_t *)malloc(ls / 2);
	m2d_frame_t f;
	uint32_t x = 12345u + (uint32_t)(w * 31 + h);
	CHECK(luma && chroma);
	for (size_t i = 0; i < ls; ++i) luma[i] = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
	for (size_t i = 0; i < ls / 2; ++i) chroma[i] = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
	memset(&f, 0, sizeof(f));
	f.luma = luma;
	f.chroma = chroma;
	f.width = (int16_t)w;
	f.height = (int16_t)h;
	memcpy(f.crop, crop, sizeof(f.crop));
	const int cw = w - crop[0] - crop[1], ch = h - crop[2] - crop[3];
	for (int filter = 0; filter < 2; ++filter)
		for (int format = M2DEC_AMD_OUT_RGB; format <= M2DEC_AMD_OUT_RGBP; ++format)
			for (int dtype = M2DEC_AMD_DT_U8; dtype <= M2DEC_AMD_DT_F32; ++dtype) {
				m2dec_amd_devout_t cfg;
				int gw = 0, gh = 0;
				memset(&cfg, 0, sizeof(cfg));
				cfg.size = sizeof(cfg);
				cfg.format = format;
				cfg.out_width = ow;
				cfg.out_height = oh;
				cfg.filter = filter;
				cfg.dtype = dtype;
				for (int c = 0; c < 3; ++c) {
					cfg.mean[c] = 0.4f + 0.03f * (float)c;
					cfg.std[c] = 0.22f + 0.01f * (float)c;
				}
				const size_t bytes = m2dec_amd_frame_out_bytes2(&cfg, cw, ch, &gw, &gh);
				CHECK(bytes == (size_t)ow * oh * 3 * (dtype == M2DEC_AMD_DT_F32 ? 4 : dtype == M2DEC_AMD_DT_F16 ? 2 : 1));
				CHECK(gw == ow && gh == oh);
				uint8_t *out = (uint8_t *)malloc(bytes);
				CHECK(out != NULL);
				CHECK(m2dec_amd_frame_convert_host(&f, &cfg, out) == 0);
				free(out);
			}
	free(luma);
	free(chroma);
}

int main(void)
{
	static const int pairs[][2] = {{16, 16}, {16, 7}, {16, 37}, {62, 9}, {130, 129}, {318, 11}, {336, 224}, {48, 224},
	                               {64, 2}, {1920, 224}, {3840, 120}};
	static const struct {
		int w, h;
		int16_t crop[4];
		int ow, oh;
	} geo[] = {
		{16, 16, {0, 0, 0, 0}, 16, 16},  {16, 16, {0, 0, 0, 0}, 7, 5},    {16, 16, {0, 0, 0, 0}, 37, 23},
		{64, 32, {0, 0, 0, 0}, 2, 1},    {144, 16, {6, 8, 0, 0}, 129, 15}, {320, 16, {2, 0, 0, 0}, 53, 16},
		{336, 48, {0, 0, 0, 0}, 224, 224}, {336, 48, {0, 0, 0, 0}, 33, 9},
	};
	for (size_t i = 0; i < sizeof(pairs) / sizeof(pairs[0]); ++i)
		for (int filter = 0; filter < 2; ++filter) taps_case(pairs[i][0], pairs[i][1], filter, 0);
	taps_case(66, 2, M2DEC_AMD_SCALE_AREA, -1);
	taps_case(66, 2, M2DEC_AMD_SCALE_BILINEAR, 0);
	for (size_t i = 0; i < sizeof(geo) / sizeof(geo[0]); ++i) convert_case(geo[i].w, geo[i].h, geo[i].crop, geo[i].ow, geo[i].oh);
	printf("BOUNDS_OK %d\n", checks);
	return 0;
}

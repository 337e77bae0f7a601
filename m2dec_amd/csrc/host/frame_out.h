/* Shared by the host restatement (frame_out.c) and the gfx950 kernel's launcher (frame_out.hip): the
 * coefficient row and the crop checks of the output conversion.  Not part of the public C ABI. */
#ifndef M2D_FRAME_OUT_H
#define M2D_FRAME_OUT_H
#include <stdint.h>
#include "m2dec_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
	int ky, yo, rv, gu, gv, bu;
} m2d_fo_coef_t;

/* cfg's coefficient row; -1 for a short / bad cfg (format, matrix) */
int m2d_frame_out_coefs(const m2dec_amd_devout_t *cfg, m2d_fo_coef_t *k);
/* the cropped size of a width x height picture; -1 for a negative or odd crop, an odd or empty result */
int m2d_frame_out_geometry(int width, int height, const int16_t crop[4], int *cw, int *ch);

/* the scale / element-type half of cfg, resolved for a cw x ch cropped picture */
typedef struct {
	int scaled;        /* 0: unscaled U8, today's conversion; 1: resample + element type (identity taps included) */
	int ow, oh;        /* output size */
	int filter, dtype;
	int esize;         /* bytes per element */
	float a[3], b[3];  /* F16 / F32: value = fmaf(q, a, b) */
} m2d_fo_scale_t;
/* -1 for every refusal of include/m2dec_amd.h that does not need the destination (the tap count included); a cfg
 * whose size does not cover the revision-7 fields resolves to unscaled U8 */
int m2d_frame_out_scale(const m2dec_amd_devout_t *cfg, int cw, int ch, m2d_fo_scale_t *s);
/* one output's taps: its first source index into *start, the weights into w[0 .. count); returns count, or -1
 * past M2DEC_AMD_SCALE_MAX_TAPS.  1 <= S, On <= 16384, 0 <= o < On, a known filter (the caller checked). */
int m2d_scale_taps_row(int S, int On, int filter, int o, int *start, uint16_t w[M2DEC_AMD_SCALE_MAX_TAPS]);

#ifdef __cplusplus
}
#endif
#endif

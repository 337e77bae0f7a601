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

#ifdef __cplusplus
}
#endif
#endif

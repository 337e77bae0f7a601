/* Stand-alone AddressSanitizer / UBSan harness for the output conversion on the host (frame_out.c), built and run by
 * tools/fuzz/run_asan.sh: every format, matrix, range and crop of the CPU test into buffers of exactly the output size. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "m2dec_amd.h"
int main(void)
{
	static const int sizes[3][2] = {{16, 16}, {32, 16}, {336, 48}};
	int n = 0;
	for (int s = 0; s < 3; ++s) {
		const int w = sizes[s][0], h = sizes[s][1];
		uint8_t *l = malloc((size_t)w * h), *c = malloc((size_t)w * h / 2);
		for (int i = 0; i < w * h; ++i) l[i] = (uint8_t)rand();
		for (int i = 0; i < w * h / 2; ++i) c[i] = (uint8_t)rand();
		const int16_t crops[6][4] = {{0, 0, 0, 0}, {2, 0, 0, 6}, {6, 4, 2, 0}, {14, 0, 14, 0}, {2, (int16_t)(w - 4), 2, (int16_t)(h - 4)}, {1, 0, 0, 0}};
		for (int k = 0; k < 6; ++k)
			for (int f = 0; f < 3; ++f)
				for (int m = 0; m < 4; ++m) {
					m2d_frame_t fr = {l, c, NULL, 0, (int16_t)w, (int16_t)h, {crops[k][0], crops[k][1], crops[k][2], crops[k][3]}};
					m2dec_amd_devout_t cfg = {sizeof(cfg), f, m & 1, m >> 1, NULL, NULL};
					const size_t bytes = m2dec_amd_frame_out_bytes(f, w - crops[k][0] - crops[k][1], h - crops[k][2] - crops[k][3]);
					uint8_t *out = malloc(bytes ? bytes : 1); /* exact size: ASan catches any overrun */
					const int r = m2dec_amd_frame_convert_host(&fr, &cfg, out);
					if ((r == 0) != (k != 5)) { printf("unexpected %d at %d %d\n", r, s, k); return 1; }
					free(out);
					++n;
				}
		free(l);
		free(c);
	}
	printf("asan ok: %d conversions\n", n);
	return 0;
}

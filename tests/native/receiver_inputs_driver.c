/* receiver_inputs_driver.c — the CPU oracle's composite (oracle/vct_oracle.c: vo_composite, the
 * one function of the oracle that starts the A.3 shadow walk from a caller's pixel) over the
 * hostile-receiver catalogue of tests/receiver_inputs.py, on several voxel fields and lights,
 * built with -fsanitize=address,undefined,float-cast-overflow (tests/native/Makefile).  A clean
 * run shows that under the "shadow-walk receiver rule" of include/vct_spec.h the reference
 * converts no float an int cannot hold (NaN, +-inf, 1e30, 2^31), reads nothing out of bounds,
 * and ends every walk, the field without the slabs included.
 * TEST INFRASTRUCTURE (tests/test_receiver_inputs.py).
 *
 * usage: receiver_inputs_driver IN OUT
 * IN : uint32 n, n_fields, n_lights, w, h; float g0[3], extent;
 *      float albedo_occ[n_fields][n^3][4]; float dir[n_lights][3], color[n_lights][3];
 *      float pos[w*h][4], nrm[w*h][4], alb[w*h][4], diffuse[w*h][4], spec[w*h][4]
 * OUT: per field, per light: float lin[w*h][4]; uint32 rgba8[w*h] */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "vct_oracle.h"

static int rd(void* p, size_t sz, size_t cnt, FILE* f) { return fread(p, sz, cnt, f) == cnt; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t hd[5];
    float fl[4];
    if (!rd(hd, 4, 5, f) || !rd(fl, 4, 4, f)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t n = hd[0], n_fields = hd[1], n_lights = hd[2], w = hd[3], h = hd[4];
    if (n < 2 || n > 64 || (n & (n - 1)) || n_fields == 0 || n_fields > 8 || n_lights == 0 || n_lights > 1024 ||
        w == 0 || h == 0 || w > 4096 || h > 4096) {
        fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const size_t nv = (size_t)n * n * n, px = (size_t)w * h;
    float* vox = malloc((size_t)n_fields * nv * 4 * sizeof(float));
    float* lights = malloc((size_t)n_lights * 6 * sizeof(float));
    float* gb = malloc(px * 20 * sizeof(float));
    float* lin = malloc(px * 4 * sizeof(float));
    uint32_t* rgba = malloc(px * sizeof(uint32_t));
    if (!vox || !lights || !gb || !lin || !rgba) return 2;
    if (!rd(vox, 4, (size_t)n_fields * nv * 4, f) || !rd(lights, 4, (size_t)n_lights * 6, f) || !rd(gb, 4, px * 20, f)) {
        fprintf(stderr, "short body\n");
        return 2;
    }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const float* dir = lights;
    const float* col = lights + (size_t)n_lights * 3;
    for (uint32_t k = 0; k < n_fields; ++k)
        for (uint32_t i = 0; i < n_lights; ++i) {
            vo_composite(n, fl, fl[3], vox + (size_t)k * nv * 4, gb, gb + px * 4, gb + px * 8, gb + px * 12, gb + px * 16,
                         w, h, dir + 3 * i, col + 3 * i, lin, rgba);
            if (fwrite(lin, 4, px * 4, f) != px * 4 || fwrite(rgba, 4, px, f) != px) return 2;
        }
    fclose(f);
    free(vox); free(lights); free(gb); free(lin); free(rgba);
    printf("ok %u %u\n", (unsigned)n_fields, (unsigned)n_lights);
    return 0;
}

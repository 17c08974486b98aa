/* light_inputs_driver.c — the CPU oracle's K2 and its composite (oracle/vct_oracle.c: vo_inject,
 * vo_composite; both run the A.3 shadow walk) over a voxel field and a list of lights read
 * from a file, built with -fsanitize=address,undefined,float-cast-overflow
 * (tests/native/Makefile).  The lights are the hostile-light catalogue of
 * tests/light_inputs.py: a clean run shows that the reference performs no undefined
 * float-to-int conversion, no out-of-bounds read and no other undefined behaviour on those
 * directions (denormal, tiny, huge) and colours (non-finite too), and ends every walk.
 * There is no light-list part: the C oracle has no light-list path (the reference of
 * vct_inject_lights is tests/lights_ref.py, in numpy), so these two functions are all of the
 * oracle's code that walks toward a light.
 * TEST INFRASTRUCTURE (tests/test_light_inputs.py).
 *
 * usage: light_inputs_driver IN OUT
 * IN : uint32 n, n_lights, w, h; float g0[3], extent;
 *      float albedo_occ[n^3][4], normal[n^3][4]; float dir[n_lights][3], color[n_lights][3];
 *      float pos[w*h][4], nrm[w*h][4], alb[w*h][4], diffuse[w*h][4], spec[w*h][4]
 * OUT: per light: float r0[n^3][4]; float lin[w*h][4]; uint32 rgba8[w*h] */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "vct_oracle.h"

static int rd(void* p, size_t sz, size_t cnt, FILE* f) { return fread(p, sz, cnt, f) == cnt; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t hd[4];
    float fl[4];
    if (!rd(hd, 4, 4, f) || !rd(fl, 4, 4, f)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t n = hd[0], n_lights = hd[1], w = hd[2], h = hd[3];
    if (n < 2 || n > 64 || (n & (n - 1)) || n_lights == 0 || n_lights > (1u << 16) || w == 0 || h == 0 ||
        w > 4096 || h > 4096) {
        fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const size_t nv = (size_t)n * n * n, px = (size_t)w * h;
    float* vox = malloc(nv * 8 * sizeof(float));
    float* lights = malloc((size_t)n_lights * 6 * sizeof(float));
    float* gb = malloc(px * 20 * sizeof(float));
    float* r0 = malloc(nv * 4 * sizeof(float));
    float* lin = malloc(px * 4 * sizeof(float));
    uint32_t* rgba = malloc(px * sizeof(uint32_t));
    if (!vox || !lights || !gb || !r0 || !lin || !rgba) return 2;
    if (!rd(vox, 4, nv * 8, f) || !rd(lights, 4, (size_t)n_lights * 6, f) || !rd(gb, 4, px * 20, f)) {
        fprintf(stderr, "short body\n");
        return 2;
    }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const float* dir = lights;
    const float* col = lights + (size_t)n_lights * 3;
    for (uint32_t i = 0; i < n_lights; ++i) {
        vo_inject(n, vox, vox + nv * 4, dir + 3 * i, col + 3 * i, r0);
        vo_composite(n, fl, fl[3], vox, gb, gb + px * 4, gb + px * 8, gb + px * 12, gb + px * 16, w, h, dir + 3 * i,
                     col + 3 * i, lin, rgba);
        if (fwrite(r0, 4, nv * 4, f) != nv * 4 || fwrite(lin, 4, px * 4, f) != px * 4 ||
            fwrite(rgba, 4, px, f) != px)
            return 2;
    }
    fclose(f);
    free(vox); free(lights); free(gb); free(r0); free(lin); free(rgba);
    printf("ok %u\n", (unsigned)n_lights);
    return 0;
}

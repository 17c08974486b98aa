/* trace_inputs_driver.c — the CPU oracle's cone trace (oracle/vct_oracle.c: vo_build_mips,
 * vo_trace) over a G-buffer read from a file, built with
 * -fsanitize=address,undefined,float-cast-overflow (tests/native/Makefile).  The frame is
 * the hostile-pixel catalogue of tests/trace_inputs.py: a clean run shows that the
 * reference performs no undefined float-to-int conversion (or other undefined behaviour)
 * on those inputs.  TEST INFRASTRUCTURE (tests/test_trace_inputs.py).
 *
 * usage: trace_inputs_driver IN OUT
 * IN : uint32 n, aniso, n_diffuse, specular, w, h; float g0[3], extent, eye[3];
 *      float r0[n^3][4], pos[h][w][4], nrm[h][w][4], alb[h][w][4]
 * OUT: float diffuse[h][w][4], spec[h][w][4]; uint32 steps_px[h][w]; uint64 cone_steps */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "vct_oracle.h"

static int rd(void* p, size_t sz, size_t cnt, FILE* f) { return fread(p, sz, cnt, f) == cnt; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t hd[6];
    float fl[7];
    if (!rd(hd, 4, 6, f) || !rd(fl, 4, 7, f)) { fprintf(stderr, "short header\n"); return 2; }
    const uint32_t n = hd[0], w = hd[4], h = hd[5];
    if (n < 2 || n > 64 || (n & (n - 1)) || w == 0 || h == 0 || w > 512 || h > 512) {
        fprintf(stderr, "bad sizes\n");
        return 2;
    }
    vo_trace_params p;
    p.n = n; p.aniso = (int)hd[1]; p.n_diffuse = hd[2]; p.specular = hd[3];
    for (int k = 0; k < 3; ++k) { p.g0[k] = fl[k]; p.eye[k] = fl[4 + k]; }
    p.extent = fl[3];
    const size_t nv = (size_t)n * n * n * 4, px = (size_t)w * h;
    float* r0 = malloc(nv * sizeof(float));
    float* gb = malloc(px * 12 * sizeof(float));
    float* pyr = malloc((vo_pyramid_floats(n, p.aniso) + 1) * sizeof(float));
    float* out = calloc(px * 8, sizeof(float));
    uint32_t* st = calloc(px, sizeof(uint32_t));
    if (!r0 || !gb || !pyr || !out || !st) return 2;
    if (!rd(r0, 4, nv, f) || !rd(gb, 4, px * 12, f)) { fprintf(stderr, "short body\n"); return 2; }
    fclose(f);
    vo_build_mips(n, p.aniso, r0, pyr);
    const uint64_t total = vo_trace(&p, r0, pyr, gb, gb + 4 * px, gb + 8 * px, w, h, 1, out, out + 4 * px, st, 1);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(out, 4, px * 8, f) != px * 8 || fwrite(st, 4, px, f) != px || fwrite(&total, 8, 1, f) != 1) return 2;
    fclose(f);
    free(r0); free(gb); free(pyr); free(out); free(st);
    printf("ok %llu\n", (unsigned long long)total);
    return 0;
}

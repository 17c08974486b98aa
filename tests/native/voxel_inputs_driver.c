/* voxel_inputs_driver.c — the CPU oracle's K1 and resolve (oracle/vct_oracle.c: vo_voxelize,
 * vo_resolve) over a mesh read from a file, built with
 * -fsanitize=address,undefined,float-cast-overflow (tests/native/Makefile).  The mesh is
 * the hostile-triangle catalogue of tests/voxel_inputs.py: a clean run shows that the
 * reference performs no undefined float-to-int conversion (or other undefined behaviour)
 * on those inputs.  TEST INFRASTRUCTURE (tests/test_voxel_inputs.py).
 *
 * usage: voxel_inputs_driver IN OUT
 * IN : uint32 n, n_verts, n_tri, n_mat; float g0[3], extent;
 *      float verts[n_verts][3]; uint32 idx[n_tri][3], mat[n_tri]; float kd[n_mat][4]
 * OUT: int32 rc; int64 sums[n^3][6]; uint32 counts[n^3]; float albedo_occ[n^3][4], normal[n^3][4] */
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
    const uint32_t n = hd[0], n_verts = hd[1], n_tri = hd[2], n_mat = hd[3];
    if (n < 2 || n > 64 || (n & (n - 1)) || n_verts > (1u << 22) || n_tri > (1u << 20) || n_mat == 0 ||
        n_mat > (1u << 20)) {
        fprintf(stderr, "bad sizes\n");
        return 2;
    }
    const size_t nv = (size_t)n * n * n;
    float* verts = malloc(((size_t)n_verts * 3 + 1) * sizeof(float));
    uint32_t* idx = malloc(((size_t)n_tri * 3 + 1) * sizeof(uint32_t));
    uint32_t* mat = malloc(((size_t)n_tri + 1) * sizeof(uint32_t));
    float* kd = malloc((size_t)n_mat * 4 * sizeof(float));
    int64_t* sums = calloc(nv * 6, sizeof(int64_t));
    uint32_t* counts = calloc(nv, sizeof(uint32_t));
    float* ao = malloc(nv * 8 * sizeof(float));
    if (!verts || !idx || !mat || !kd || !sums || !counts || !ao) return 2;
    if (!rd(verts, 4, (size_t)n_verts * 3, f) || !rd(idx, 4, (size_t)n_tri * 3, f) || !rd(mat, 4, n_tri, f) ||
        !rd(kd, 4, (size_t)n_mat * 4, f)) {
        fprintf(stderr, "short body\n");
        return 2;
    }
    fclose(f);
    const int32_t rc = vo_voxelize(n, fl, fl[3], verts, 12, n_verts, idx, n_tri * 3, mat, kd, n_mat, sums, counts);
    vo_resolve(n, sums, counts, ao, ao + nv * 4);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(&rc, 4, 1, f) != 1 || fwrite(sums, 8, nv * 6, f) != nv * 6 || fwrite(counts, 4, nv, f) != nv ||
        fwrite(ao, 4, nv * 8, f) != nv * 8)
        return 2;
    fclose(f);
    free(verts); free(idx); free(mat); free(kd); free(sums); free(counts); free(ao);
    printf("ok %d\n", (int)rc);
    return 0;
}

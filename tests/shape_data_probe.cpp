// Host program of tests/test_shape_data_cpu.py: the argument checks and the host image of the shape-data builder
// (csrc/sm_shape_data.h) without a GPU.
//   shape_data_probe IN P T LOSS   IN = int64 B, vert_off (B + 1) int64, face_off (B + 1) int64, verts float64, faces int32
// Prints "error <message>" and returns 1 when the checks refuse the batch; else one line per value, "%.17g":
//   cdf f value | lohi b (6 values) | pbounds b (5 values) | off b face_off vert_off
#define SM_SHAPE_DATA_HOST_ONLY
#include "../shapemol_amd/csrc/sm_shape_data.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    int64_t B = 0;
    if (!f || std::fread(&B, 8, 1, f) != 1 || B < 0 || B > 4096) return 2;
    std::vector<int64_t> vo(B + 1), fo(B + 1);
    if (std::fread(vo.data(), 8, B + 1, f) != (size_t)B + 1 || std::fread(fo.data(), 8, B + 1, f) != (size_t)B + 1) return 2;
    if (vo[B] < 0 || fo[B] < 0 || vo[B] > (1 << 24) || fo[B] > (1 << 24)) return 2;
    const size_t nv = (size_t)vo[B] * 3, nf = (size_t)fo[B] * 3;
    std::vector<double> verts(nv + 1);                  // (one spare element: an empty batch still has a pointer to give)
    std::vector<int32_t> faces(nf + 1);
    if (std::fread(verts.data(), 8, nv, f) != nv || std::fread(faces.data(), 4, nf, f) != nf || std::fgetc(f) != EOF) return 2;
    std::fclose(f);
    const std::string e = sdata_check(B, vo.data(), verts.data(), fo.data(), faces.data(), std::atoll(argv[2]), std::atoll(argv[3]), std::atoi(argv[4]));
    if (!e.empty()) { std::printf("error %s\n", e.c_str()); return 1; }
    SdataImage im;
    sdata_image((int)B, vo.data(), verts.data(), fo.data(), faces.data(), im);
    const unsigned char *base = im.bytes.data();
    const double *cdf = reinterpret_cast<const double *>(base + im.o_cdf), *pb = reinterpret_cast<const double *>(base + im.o_pb);
    const double *lohi = reinterpret_cast<const double *>(base + im.o_lohi);
    const int *off = reinterpret_cast<const int *>(base + im.o_off), *voff = reinterpret_cast<const int *>(base + im.o_voff);
    for (int64_t i = 0; i < im.F; ++i) {
        std::printf("cdf %lld %.17g\n", (long long)i, cdf[i]);
    }
    for (int64_t b = 0; b < B; ++b) {
        std::printf("lohi %lld", (long long)b);
        for (int k = 0; k < 6; ++k) std::printf(" %.17g", lohi[6 * b + k]);
        std::printf("\npbounds %lld", (long long)b);
        for (int k = 0; k < 5; ++k) std::printf(" %.17g", pb[5 * b + k]);
        std::printf("\n");
    }
    for (int64_t b = 0; b <= B; ++b) std::printf("off %lld %d %d\n", (long long)b, off[b], voff[b]);
    return 0;
}

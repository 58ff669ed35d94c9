// Evaluates mm_atan2f / mm_asinf of include/miro_math.h on the host for tests/test_environment.py: reads n pairs of floats
// (a, b) and writes, per pair, mm_atan2f(a, b) and mm_asinf(a).
//
// usage: env_math <pairs.bin> <out.bin>
#include <cstdio>
#include <vector>

#include "miro_math.h"

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 3;
    fseek(fp, 0, SEEK_END);
    const size_t n = (size_t)ftell(fp) / 8;
    fseek(fp, 0, SEEK_SET);
    std::vector<float> in(2 * n), out(2 * n);
    if (fread(in.data(), 8, n, fp) != n) return 4;
    fclose(fp);
    for (size_t i = 0; i < n; i++) {
        out[2 * i] = mm_atan2f(in[2 * i], in[2 * i + 1]);
        out[2 * i + 1] = mm_asinf(in[2 * i]);
    }
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 5;
    fwrite(out.data(), 8, n, fo);
    fclose(fo);
    return 0;
}

// lm_solve_main.cpp -- runs lm_device.h's cholesky_solve on the host, for
// tests/test_lm_core.py to compare with tests/lm_ref.py byte for byte.
//   lm_solve_main <in.bin> <out.bin>
// in:  float64 N (6 or 7), the N (N + 1) / 2 upper entries of H row by row, b (N), lambda
// out: float64 1 and x (N) when the solve succeeded, float64 0 alone when a pivot failed
#include <cstdio>
#include <vector>

#include "../../orb-slam2-annotation_amd/csrc/lm_device.h"

template <int N>
static std::vector<double> solve(const double* in) {
    constexpr int U = N * (N + 1) / 2;
    double x[N], L[U], y[N];
    if (!orbgpu::lm::cholesky_solve<N>(in, in + U, in[U + N], x, L, y)) return {0.0};
    std::vector<double> out = {1.0};
    out.insert(out.end(), x, x + N);
    return out;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: lm_solve_main <in.bin> <out.bin>\n");
        return 2;
    }
    std::vector<double> in(1 + 28 + 7 + 1);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const size_t got = std::fread(in.data(), sizeof(double), in.size(), f);
    std::fclose(f);
    const int n = got ? (int)in[0] : 0;
    if ((n != 6 && n != 7) || got != (size_t)(1 + n * (n + 1) / 2 + n + 1)) {
        std::fprintf(stderr, "lm_solve_main: N = 6 or 7 and N (N + 1) / 2 + N + 1 values after it\n");
        return 2;
    }
    const std::vector<double> out = n == 6 ? solve<6>(in.data() + 1) : solve<7>(in.data() + 1);
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}

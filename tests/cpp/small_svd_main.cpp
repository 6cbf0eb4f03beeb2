// small_svd_main.cpp -- runs csrc/small_svd.h's Jacobis and csrc/epnp.h's
// qr_solve_6x4 on the host, for tests/test_small_svd.py.
//   small_svd_main <mode> <in.bin> <out.bin>
// Both files are float64 records, as many as the input holds:
//   qr    A (6 x 4), b (6), X0 (4)          -> X (4) after qr_solve_6x4
//   zero  L (6 x 10), rho (6)               -> svd_solve<6,5> of [L0 L1 L3 L6 0] (5), svd_solve<6,4> of
//                                              [L0 L1 L3 L6] (4), svd_solve<6,5> of [L0 L1 L2 0 0] (5),
//                                              svd_solve<6,3> of [L0 L1 L2] (3)
//   svd3  A (3 x 3)                         -> s (3), V (3 x 3), U s (3 x 3) of svd_hestenes<3,3>
//   svd4  A (4 x 4)                         -> s (4), V (4 x 4), U s (4 x 4) of svd_hestenes<4,4>
//   eig3  symmetric A (3 x 3)               -> w (3), ut (3 x 3) of sym_eig_desc<3>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../orb-slam2-annotation_amd/csrc/epnp.h"

using namespace orbgpu;

// columns cols[0..NC) of L (6 x 10) as a 6 x N system, the columns past NC zero
template <int N>
static void solve_columns(const double* L, const double* rho, const int* cols, int nc, std::vector<double>& out) {
    double l[6 * N], x[N];
    for (int i = 0; i < 6; ++i)
        for (int k = 0; k < N; ++k) l[N * i + k] = k < nc ? L[10 * i + cols[k]] : 0.0;
    svd_solve<6, N>(l, rho, x);
    out.insert(out.end(), x, x + N);
}

template <int N>
static void svd(const double* in, std::vector<double>& out) {
    double a[N * N], s[N], v[N * N];
    std::memcpy(a, in, sizeof a);
    svd_hestenes<N, N>(a, s, v);
    out.insert(out.end(), s, s + N);
    out.insert(out.end(), v, v + N * N);
    out.insert(out.end(), a, a + N * N);
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: small_svd_main qr|zero|svd3|svd4|eig3 <in.bin> <out.bin>\n");
        return 2;
    }
    const char* modes[] = {"qr", "zero", "svd3", "svd4", "eig3"};
    const size_t widths[] = {34, 66, 9, 16, 9};
    int mode = -1;
    for (int m = 0; m < 5; ++m)
        if (!std::strcmp(argv[1], modes[m])) mode = m;
    FILE* f = mode < 0 ? nullptr : std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<double> in, out;
    double buf[66];
    const size_t w = widths[mode];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), w, f)) == w) in.insert(in.end(), buf, buf + w);
    std::fclose(f);
    if (got != 0 || in.empty()) {
        std::fprintf(stderr, "small_svd_main: %s takes whole records of %zu values\n", argv[1], w);
        return 2;
    }
    for (const double* p = in.data(); p < in.data() + in.size(); p += w) {
        if (mode == 0) {
            double A[24], b[6], X[4];
            std::memcpy(A, p, sizeof A);
            std::memcpy(b, p + 24, sizeof b);
            std::memcpy(X, p + 30, sizeof X);
            epnp::qr_solve_6x4(A, b, X);
            out.insert(out.end(), X, X + 4);
        } else if (mode == 1) {
            const int c1[4] = {0, 1, 3, 6}, c2[3] = {0, 1, 2};
            solve_columns<5>(p, p + 60, c1, 4, out);
            solve_columns<4>(p, p + 60, c1, 4, out);
            solve_columns<5>(p, p + 60, c2, 3, out);
            solve_columns<3>(p, p + 60, c2, 3, out);
        } else if (mode == 2) {
            svd<3>(p, out);
        } else if (mode == 3) {
            svd<4>(p, out);
        } else {
            double a[9], wv[3], ut[9];
            std::memcpy(a, p, sizeof a);
            sym_eig_desc<3>(a, wv, ut);
            out.insert(out.end(), wv, wv + 3);
            out.insert(out.end(), ut, ut + 9);
        }
    }
    f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}

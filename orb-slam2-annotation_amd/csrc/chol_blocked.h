// chol_blocked.h -- the dense blocked Cholesky and the column-oriented
// back-substitution of a system whose size is known at run time only, driven a
// launch per phase over the whole chip: globalba.hip's reduced
// pose system and essential.hip's 7-dof pose graph.  The matrix is kept as its
// lower triangle in rows of n doubles, the right-hand side being row n: its
// factor row is y, and the back-substitution turns it into the running s.
//
//   entry (i, j) of the factor      A(i, j) - sum_k L(i, k) L(j, k) in ascending k: panel by panel in
//                                   the trailing update, then inside its own panel; the bits do not
//                                   depend on kNB or the tiling and equal the unblocked loop's
//   s[k] of the back-substitution   s[k] -= L(i, k) x[i] in descending i
// A pivot that is not positive sets the fail word; every later kernel returns at once on it.
// tests/globalba_ref.py's blocked_order_solve is the same arithmetic.
//
// The kernels are templates over a view of the four things they read:
//   double* S, double* x            the matrix with its extra row, the solution
//   size_t n() const                the system's size, read on the device
//   int* fail                       the word a failed pivot sets
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace orbgpu {
namespace chol {

constexpr int kNB = 48;    // panel width of the factorisation
constexpr int kTile = 16;  // the trailing update works on kTile x kTile entries per workgroup
constexpr int kRows = 64;  // rows per workgroup of the panel solve
constexpr int kBackThreads = 256;

// step 1, one workgroup: the diagonal block, column by column; a pivot that is not positive sets fail
template <class View>
__global__ __launch_bounds__(64) void diag(View A, int c0, int w) {
    __shared__ double D[kNB][kNB + 1];
    __shared__ double s_r[kNB];
    if (*A.fail) return;
    const size_t n = A.n();
    const int i = threadIdx.x;
    if (i < w)
        for (int j = 0; j <= i; ++j) D[i][j] = A.S[(size_t)(c0 + i) * n + c0 + j];
    __syncthreads();
    for (int j = 0; j < w; ++j) {
        if (i >= j && i < w) {
            double r = D[i][j];
            for (int k = 0; k < j; ++k) r -= D[i][k] * D[j][k];
            s_r[i] = r;
        }
        __syncthreads();
        const double pivot = s_r[j];
        if (!(pivot > 0)) {  // every lane read the same word
            if (i == 0) *A.fail = 1;
            return;
        }
        const double d = __dsqrt_rn(pivot);
        if (i == j) D[j][j] = d;
        if (i > j && i < w) D[i][j] = s_r[i] / d;
        __syncthreads();
    }
    if (i < w)
        for (int j = 0; j <= i; ++j) A.S[(size_t)(c0 + i) * n + c0 + j] = D[i][j];
}

// step 2, one lane per row below the block (the right-hand side's row included): its row of the panel
template <class View>
__global__ __launch_bounds__(kRows) void panel(View A, int c0, int w) {
    __shared__ double D[kNB][kNB + 1];
    __shared__ double Rw[kRows][kNB + 1];
    if (*A.fail) return;
    const size_t n = A.n();
    const int t = threadIdx.x;
    for (int v = t; v < w * w; v += kRows) {
        const int a = v / w, b = v % w;
        if (b <= a) D[a][b] = A.S[(size_t)(c0 + a) * n + c0 + b];
    }
    const size_t row = (size_t)c0 + w + (size_t)blockIdx.x * kRows + t;
    const bool live = row <= n;
    if (live)
        for (int j = 0; j < w; ++j) Rw[t][j] = A.S[row * n + c0 + j];
    __syncthreads();
    if (!live) return;
    for (int j = 0; j < w; ++j) {
        double s = Rw[t][j];
        for (int k = 0; k < j; ++k) s -= Rw[t][k] * D[j][k];
        s = s / D[j][j];
        Rw[t][j] = s;
        A.S[row * n + c0 + j] = s;
    }
}

// step 3, the trailing update: entry (i, j), c0 + w <= j <= i <= n, loses sum_k L(i, k) L(j, k) over the
// panel's columns in ascending k, from panel rows staged in LDS
template <class View>
__global__ __launch_bounds__(kTile* kTile) void update(View A, int c0, int w) {
    __shared__ double Li[kTile][kNB + 1];
    __shared__ double Lj[kTile][kNB + 1];
    if (*A.fail) return;
    if (blockIdx.x > blockIdx.y) return;  // tiles above the diagonal
    const size_t n = A.n();
    const size_t c1 = (size_t)c0 + w;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    const size_t i0 = c1 + (size_t)blockIdx.y * kTile, j0 = c1 + (size_t)blockIdx.x * kTile;
    for (int k = tx; k < w; k += kTile) {
        Li[ty][k] = i0 + ty <= n ? A.S[(i0 + ty) * n + c0 + k] : 0.0;
        Lj[ty][k] = j0 + ty < n ? A.S[(j0 + ty) * n + c0 + k] : 0.0;
    }
    __syncthreads();
    const size_t i = i0 + ty, j = j0 + tx;
    if (i > n || j >= n || j > i) return;
    double s = A.S[i * n + j];
    for (int k = 0; k < w; ++k) s -= Li[ty][k] * Lj[tx][k];
    A.S[i * n + j] = s;
}

// L^T x = y, column oriented, panels descending; y is row n of the matrix and becomes the running s.
// One workgroup solves the panel's own block ...
template <class View>
__global__ __launch_bounds__(64) void back_diag(View A, int c0, int w) {
    __shared__ double D[kNB][kNB + 1];
    __shared__ double s_s[kNB];
    __shared__ double s_x;
    if (*A.fail) return;
    const size_t n = A.n();
    const int k = threadIdx.x;
    if (k < w) {
        for (int j = 0; j <= k; ++j) D[k][j] = A.S[(size_t)(c0 + k) * n + c0 + j];
        s_s[k] = A.S[n * n + c0 + k];
    }
    __syncthreads();
    for (int i = w - 1; i >= 0; --i) {
        if (k == i) {
            s_x = s_s[i] / D[i][i];
            A.x[c0 + i] = s_x;
        }
        __syncthreads();
        if (k < i) s_s[k] -= D[i][k] * s_x;
        __syncthreads();
    }
}

// ... then one lane per row above it takes the panel's x out of its s, i descending
template <class View>
__global__ __launch_bounds__(kBackThreads) void back_rows(View A, int c0, int w) {
    __shared__ double s_x[kNB];
    if (*A.fail) return;
    const size_t n = A.n();
    if ((int)threadIdx.x < w) s_x[threadIdx.x] = A.x[c0 + threadIdx.x];
    __syncthreads();
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (size_t)c0) return;
    double s = A.S[n * n + k];
    for (int i = w - 1; i >= 0; --i) s -= A.S[(size_t)(c0 + i) * n + k] * s_x[i];
    A.S[n * n + k] = s;
}

inline unsigned blocks_for(size_t lanes, int threads) { return (unsigned)((lanes + threads - 1) / threads); }

// Enqueues the factorisation and the back-substitution of the n x n system in `view` on `st`; n > 0 is
// the host's copy of view.n().  Returns the first launch error.
template <class View>
inline hipError_t enqueue_solve(const View& view, size_t n, hipStream_t st) {
#define CHOL_LAUNCH(kernel, grid, block, ...)                                   \
    do {                                                                        \
        hipLaunchKernelGGL(kernel<View>, grid, block, 0, st, view, __VA_ARGS__); \
        if (hipError_t e = hipGetLastError()) return e;                         \
    } while (0)
    for (size_t c0 = 0; c0 < n; c0 += kNB) {
        const int w = (int)(n - c0 < (size_t)kNB ? n - c0 : (size_t)kNB);
        const size_t below = n + 1 - (c0 + w);  // rows under the block, the right-hand side's included
        CHOL_LAUNCH(diag, dim3(1), dim3(64), (int)c0, w);
        CHOL_LAUNCH(panel, dim3(blocks_for(below, kRows)), dim3(kRows), (int)c0, w);
        if (c0 + w == n) break;  // no column is left
        const unsigned tiles = blocks_for(below, kTile);
        CHOL_LAUNCH(update, dim3(tiles, tiles), dim3(kTile * kTile), (int)c0, w);
    }
    for (size_t c0 = ((n - 1) / kNB) * kNB;; c0 -= kNB) {
        const int w = (int)(n - c0 < (size_t)kNB ? n - c0 : (size_t)kNB);
        CHOL_LAUNCH(back_diag, dim3(1), dim3(64), (int)c0, w);
        if (c0 == 0) break;
        CHOL_LAUNCH(back_rows, dim3(blocks_for(c0, kBackThreads)), dim3(kBackThreads), (int)c0, w);
    }
#undef CHOL_LAUNCH
    return hipSuccess;
}

}  // namespace chol
}  // namespace orbgpu

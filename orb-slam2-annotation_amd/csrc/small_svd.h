// small_svd.h -- the sequential Jacobi decompositions of small dense
// matrices, one matrix per thread, host and device: the symmetric
// eigen-decomposition (cyclic Jacobi, eigenvalues sorted descending) for
// symmetric PSD matrices, the one-sided (Hestenes) Jacobi SVD for general
// ones, and the pseudo-inverse solve built on it.  They restate the
// reference's OpenCV calls (cvSVD of a symmetric matrix, cv::SVDecomp,
// cvInvert / cvSolve with CV_SVD) for EPnP (epnp.h), the Initializer's
// triangulation and normalisation (init_models.hip, init_reconstruct.hip) and
// local mapping's triangulation (mapping.hip).  The rotation is
// jacobi_group.h's jacobi_rot: IEEE on the host, the fast reciprocals on the
// device.
#pragma once

#include <hip/hip_runtime.h>

#include "jacobi_group.h"

namespace orbgpu {

// cyclic Jacobi on symmetric n x n `a` (row-major, destroyed); eigenvalues
// to w[0..n) and eigenvectors to the ROWS of ut, sorted by descending
// eigenvalue (cvSVD(..., CV_SVD_U_T) of a symmetric PSD matrix).
template <int N>
__host__ __device__ void sym_eig_desc(double* a, double* w, double* ut) {
    double v[N * N];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) v[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < N; ++i) {
            diag += a[i * N + i] * a[i * N + i];
            for (int j = i + 1; j < N; ++j) off += a[i * N + j] * a[i * N + j];
        }
        if (off <= 1e-32 * diag || off == 0.0) break;
#pragma unroll
        for (int p = 0; p < N - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = a[p * N + q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (a[q * N + q] - a[p * N + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) {
                    const double akp = a[k * N + p], akq = a[k * N + q];
                    a[k * N + p] = c * akp - s * akq;
                    a[k * N + q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; ++k) {
                    const double apk = a[p * N + k], aqk = a[q * N + k];
                    a[p * N + k] = c * apk - s * aqk;
                    a[q * N + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < N; ++k) {
                    const double vkp = v[k * N + p], vkq = v[k * N + q];
                    v[k * N + p] = c * vkp - s * vkq;
                    v[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
    // descending by eigenvalue, stable (the order of an insertion sort that
    // moves an entry before strictly smaller ones): column c goes to rank
    // #{j : w_j > w_c} + #{j < c : w_j == w_c}; selected with constant
    // indices only (a dynamic order[] put a, v, w and ut in scratch memory)
#pragma unroll
    for (int c = 0; c < N; ++c) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            rank += (a[j * N + j] > a[c * N + c]) || (j < c && a[j * N + j] == a[c * N + c]);
#pragma unroll
        for (int r = 0; r < N; ++r)
            if (rank == r) {
                w[r] = a[c * N + c];
#pragma unroll
                for (int k = 0; k < N; ++k) ut[r * N + k] = v[k * N + c];
            }
    }
}

// one-sided Jacobi SVD of m x n `a` (m >= n, row-major): on return the
// columns of a are U_j * sigma_j, sigma in s[], V in v (n x n, row-major)
template <int M, int N>
__host__ __device__ void svd_hestenes(double* a, double* s, double* v) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) v[i * N + j] = i == j ? 1.0 : 0.0;
    double fro = 0.0;  // numerically null columns take no rotation (jacobi_group.h)
    for (int k = 0; k < M * N; ++k) fro += a[k] * a[k];
    const double negl = kJacobiNegl * fro;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        // fully unrolled (device): constant indices keep a and v in registers
#pragma unroll
        for (int p = 0; p < N - 1; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    alpha += a[k * N + p] * a[k * N + p];
                    beta += a[k * N + q] * a[k * N + q];
                    gamma += a[k * N + p] * a[k * N + q];
                }
                double c, sn;
                if (!jacobi_rot(alpha, beta, gamma, negl, c, sn)) continue;
                rotated = true;
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    const double x = a[k * N + p], y = a[k * N + q];
                    a[k * N + p] = c * x - sn * y;
                    a[k * N + q] = sn * x + c * y;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double x = v[k * N + p], y = v[k * N + q];
                    v[k * N + p] = c * x - sn * y;
                    v[k * N + q] = sn * x + c * y;
                }
            }
        if (!rotated) break;
    }
    for (int j = 0; j < N; ++j) {
        double nrm = 0.0;
        for (int k = 0; k < M; ++k) nrm += a[k * N + j] * a[k * N + j];
        s[j] = sqrt(nrm);
    }
}

// x = pinv(A) b for m x n A (cvSolve(A, b, x, CV_SVD)); A is destroyed
template <int M, int N>
__host__ __device__ void svd_solve(double* A, const double* b, double* x) {
    double s[N], v[N * N];
    svd_hestenes<M, N>(A, s, v);
    double smax = 0.0;
    for (int j = 0; j < N; ++j) smax = fmax(smax, s[j]);
    const double thr = smax * 2.220446049250313e-16 * M;
    double y[N];
    for (int j = 0; j < N; ++j) {  // y = Sigma^+ U^T b, U_j = a_j / s_j
        double d = 0.0;
        if (s[j] > thr) {
            for (int k = 0; k < M; ++k) d += A[k * N + j] * b[k];
            d /= s[j] * s[j];
        }
        y[j] = d;
    }
    for (int i = 0; i < N; ++i) {
        double acc = 0.0;
        for (int j = 0; j < N; ++j) acc += v[i * N + j] * y[j];
        x[i] = acc;
    }
}

}  // namespace orbgpu

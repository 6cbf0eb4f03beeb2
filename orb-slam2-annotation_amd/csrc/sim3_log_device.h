// sim3_log_device.h -- g2o's Sim3::log (types/sim3.h:148-230, with deltaR and
// skew of se3_ops.hpp:27-47) and Sim3::map (:144-146) in double, beside
// sim3opt_device.h's Sim3(Vector7d), product and inverse: what essential.hip
// needs of the type and sim3opt.hip does not.  tests/essential_ref.py's
// sim3_log is the same arithmetic, expression for expression.  Everything is
// indexed at compile time, so a lane keeps its values in registers.
#pragma once

#include <hip/hip_runtime.h>

#include "se3_device.h"
#include "sim3opt_device.h"

namespace orbgpu {
namespace sim3opt {

using se3::quat_to_R;  // Eigen's Quaternion::toRotationMatrix of q = (x, y, z, w), not normalised

// W x = t by elimination with partial pivoting, the first largest |entry| of the column; the
// order is tests/essential_ref.py's (Eigen's W.lu().solve(t) is restated, not reproduced)
__device__ inline void lu_solve3(const double (&W)[3][3], const double (&t)[3], double (&x)[3]) {
    double r0[4] = {W[0][0], W[0][1], W[0][2], t[0]};
    double r1[4] = {W[1][0], W[1][1], W[1][2], t[1]};
    double r2[4] = {W[2][0], W[2][1], W[2][2], t[2]};
    const double a0 = fabs(r0[0]), a1 = fabs(r1[0]), a2 = fabs(r2[0]);
    const bool p1 = a1 > a0;
    const bool p2 = a2 > (p1 ? a1 : a0);
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // row 0 <-> the pivot's row
        const double v0 = r0[c], v1 = r1[c], v2 = r2[c];
        r0[c] = p2 ? v2 : (p1 ? v1 : v0);
        r1[c] = (!p2 && p1) ? v0 : v1;
        r2[c] = p2 ? v0 : v2;
    }
    const double f1 = r1[0] / r0[0], f2 = r2[0] / r0[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        r1[c] = r1[c] - f1 * r0[c];
        r2[c] = r2[c] - f2 * r0[c];
    }
    const bool swap = fabs(r2[1]) > fabs(r1[1]);
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const double v1 = r1[c], v2 = r2[c];
        r1[c] = swap ? v2 : v1;
        r2[c] = swap ? v1 : v2;
    }
    const double f = r2[1] / r1[1];
    const double r22 = r2[2] - f * r1[2];
    const double r23 = r2[3] - f * r1[3];
    x[2] = r23 / r22;
    x[1] = (r1[3] - r1[2] * x[2]) / r1[1];
    x[0] = ((r0[3] - r0[1] * x[1]) - r0[2] * x[2]) / r0[0];
}

// Sim3::log as written: out = (omega, upsilon, sigma).  The branch |sigma| >= eps, d > 1 - eps keeps
// the B of Sim3(Vector7d)'s same branch.
__device__ inline void sim3_log(const Sim3& S, double (&out)[7]) {
    const double s = S.s;
    const double sigma = log(s);
    double R[3][3];
    quat_to_R(S.q, R);
    const double d = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1.0);
    const double eps = lm::kSmallAngle;
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    const bool near = d > 1.0 - eps;
    double A, B, C, k;
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (near) {
            k = 0.5;
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            const double theta = acos(d);
            const double theta2 = theta * theta;
            k = theta / (2.0 * __dsqrt_rn(1.0 - d * d));
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (near) {
            const double sigma2 = sigma * sigma;
            k = 0.5;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            k = theta / (2.0 * __dsqrt_rn(1.0 - d * d));
            const double theta2 = theta * theta;
            const double a = s * sin(theta);
            const double b = s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    const double om[3] = {k * dR[0], k * dR[1], k * dR[2]};
    const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    double W[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {  // A Omega + (B Omega) Omega + C I
            const double boo = ((B * O[i][0]) * O[0][j] + (B * O[i][1]) * O[1][j]) + (B * O[i][2]) * O[2][j];
            W[i][j] = (A * O[i][j] + boo) + C * (i == j ? 1.0 : 0.0);
        }
    double up[3];
    lu_solve3(W, S.t, up);
    out[0] = om[0], out[1] = om[1], out[2] = om[2];
    out[3] = up[0], out[4] = up[1], out[5] = up[2];
    out[6] = sigma;
}

// Sim3::map: s * (r * xyz) + t
__device__ inline void sim3_map(const Sim3& S, const double (&p)[3], double (&out)[3]) {
    double r0, r1, r2;
    lm::quat_rotate(S.q, p[0], p[1], p[2], r0, r1, r2);
    out[0] = S.s * r0 + S.t[0];
    out[1] = S.s * r1 + S.t[1];
    out[2] = S.s * r2 + S.t[2];
}

}  // namespace sim3opt
}  // namespace orbgpu

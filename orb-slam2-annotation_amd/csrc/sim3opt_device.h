// sim3opt_device.h -- g2o's Sim3 (types/sim3.h) in double, for sim3opt.hip
// alone, on the quaternion algebra and the Rodrigues block of lm_device.h;
// everything is indexed at compile time, so a lane keeps its values in
// registers.
#pragma once

#include <hip/hip_runtime.h>

#include "lm_device.h"

namespace orbgpu {
namespace sim3opt {

struct Sim3 {
    double q[4];  // x, y, z, w
    double t[3];
    double s;
};

// Sim3(const Vector7d& update)  (sim3.h:70-142), update = (omega, upsilon, sigma)
__device__ inline void sim3_exp(const double (&u)[7], Sim3& out) {
    const double sigma = u[6];
    double O[3][3], O2[3][3], R[9];
    const double theta = lm::rodrigues(u[0], u[1], u[2], O, O2, R);
    const double s = exp(sigma);
    const double eps = lm::kSmallAngle;
    double A, B, C;
    const bool small_angle = theta < eps;
    if (fabs(sigma) < eps) {
        C = 1.0;
        if (small_angle) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small_angle) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta);
            const double b = s * cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.0) / theta2;
        }
    }
    lm::quat_from_R(R, out.q);  // not normalised
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double W[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) W[j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
        out.t[i] = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
    }
    out.s = s;
}

// Sim3::operator*  (sim3.h:266-272): the quaternion product is not normalised
__device__ inline void sim3_mul(const Sim3& a, const Sim3& b, Sim3& out) {
    double r0, r1, r2;
    lm::quat_rotate(a.q, b.t[0], b.t[1], b.t[2], r0, r1, r2);
    lm::quat_mul(a.q, b.q, out.q);
    out.t[0] = a.s * r0 + a.t[0];
    out.t[1] = a.s * r1 + a.t[1];
    out.t[2] = a.s * r2 + a.t[2];
    out.s = a.s * b.s;
}

// Sim3::inverse  (sim3.h:233-236)
__device__ inline void sim3_inverse(const Sim3& a, Sim3& out) {
    const double qc[4] = {-a.q[0], -a.q[1], -a.q[2], a.q[3]};
    const double c = -1.0 / a.s;
    double r0, r1, r2;
    lm::quat_rotate(qc, c * a.t[0], c * a.t[1], c * a.t[2], r0, r1, r2);
#pragma unroll
    for (int i = 0; i < 4; ++i) out.q[i] = qc[i];
    out.t[0] = r0, out.t[1] = r1, out.t[2] = r2;
    out.s = 1.0 / a.s;
}

}  // namespace sim3opt
}  // namespace orbgpu

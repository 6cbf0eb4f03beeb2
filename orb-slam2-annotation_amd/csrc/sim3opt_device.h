// sim3opt_device.h -- g2o's Sim3 (types/sim3.h) and the Eigen quaternion
// algebra it uses, in double, for sim3opt.hip alone.  The three quaternion
// helpers restate the same Eigen functions as poseopt.hip's; everything is
// indexed at compile time, so a lane keeps its values in registers.
#pragma once

#include <hip/hip_runtime.h>

namespace orbgpu {
namespace sim3opt {

struct Sim3 {
    double q[4];  // x, y, z, w
    double t[3];
    double s;
};

template <int I>
__device__ __forceinline__ void quat_from_R_branch(const double (&R)[9], double (&q)[4]) {
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = __dsqrt_rn(((R[4 * I] - R[4 * J]) - R[4 * K]) + 1.0);
    q[I] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[3 * K + J] - R[3 * J + K]) * t;
    q[J] = (R[3 * J + I] + R[3 * I + J]) * t;
    q[K] = (R[3 * K + I] + R[3 * I + K]) * t;
}

// Eigen: Quaterniond(Matrix3d), R row-major
__device__ inline void quat_from_R(const double (&R)[9], double (&q)[4]) {
    double t = (R[0] + R[4]) + R[8];
    if (t > 0) {
        t = __dsqrt_rn(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t;
        q[1] = (R[2] - R[6]) * t;
        q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i == 1 ? R[4] : R[0])) i = 2;
        if (i == 0)
            quat_from_R_branch<0>(R, q);
        else if (i == 1)
            quat_from_R_branch<1>(R, q);
        else
            quat_from_R_branch<2>(R, q);
    }
}

// Eigen's Quaternion::_transformVector
__device__ __forceinline__ void quat_rotate(const double (&q)[4], double v0, double v1, double v2, double& r0,
                                            double& r1, double& r2) {
    double ux = q[1] * v2 - q[2] * v1;
    double uy = q[2] * v0 - q[0] * v2;
    double uz = q[0] * v1 - q[1] * v0;
    ux = ux + ux, uy = uy + uy, uz = uz + uz;
    r0 = (v0 + q[3] * ux) + (q[1] * uz - q[2] * uy);
    r1 = (v1 + q[3] * uy) + (q[2] * ux - q[0] * uz);
    r2 = (v2 + q[3] * uz) + (q[0] * uy - q[1] * ux);
}

// Sim3(const Vector7d& update)  (sim3.h:70-142), update = (omega, upsilon, sigma)
__device__ inline void sim3_exp(const double (&u)[7], Sim3& out) {
    const double om0 = u[0], om1 = u[1], om2 = u[2];
    const double sigma = u[6];
    const double theta = __dsqrt_rn((om0 * om0 + om1 * om1) + om2 * om2);
    const double O[3][3] = {{0.0, -om2, om1}, {om2, 0.0, -om0}, {-om1, om0, 0.0}};
    const double s = exp(sigma);
    double O2[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
    const double eps = 0.00001;
    double A, B, C;
    bool small_angle = theta < eps;
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
    double R[9];
    if (small_angle) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[3 * i + j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
    } else {
        const double ra = sin(theta) / theta;
        const double rb = (1.0 - cos(theta)) / (theta * theta);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[3 * i + j] = ((i == j ? 1.0 : 0.0) + ra * O[i][j]) + rb * O2[i][j];
    }
    quat_from_R(R, out.q);  // not normalised
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
    quat_rotate(a.q, b.t[0], b.t[1], b.t[2], r0, r1, r2);
    const double* aq = a.q;
    const double* bq = b.q;
    const double q0 = ((aq[3] * bq[0] + aq[0] * bq[3]) + aq[1] * bq[2]) - aq[2] * bq[1];
    const double q1 = ((aq[3] * bq[1] + aq[1] * bq[3]) + aq[2] * bq[0]) - aq[0] * bq[2];
    const double q2 = ((aq[3] * bq[2] + aq[2] * bq[3]) + aq[0] * bq[1]) - aq[1] * bq[0];
    const double q3 = ((aq[3] * bq[3] - aq[0] * bq[0]) - aq[1] * bq[1]) - aq[2] * bq[2];
    out.q[0] = q0, out.q[1] = q1, out.q[2] = q2, out.q[3] = q3;
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
    quat_rotate(qc, c * a.t[0], c * a.t[1], c * a.t[2], r0, r1, r2);
#pragma unroll
    for (int i = 0; i < 4; ++i) out.q[i] = qc[i];
    out.t[0] = r0, out.t[1] = r1, out.t[2] = r2;
    out.s = 1.0 / a.s;
}

}  // namespace sim3opt
}  // namespace orbgpu

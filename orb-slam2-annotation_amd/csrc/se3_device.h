// se3_device.h -- g2o's SE3Quat (types/se3quat.h) over (q[4], t[3]) arrays in
// double, q = (x, y, z, w): normalizeRotation, exp(x) * pose, Eigen's
// toRotationMatrix and Converter::toSE3Quat of a 3x4 float Tcw.  One copy for
// localba.hip and globalba.hip (and quat_to_R for sim3_log_device.h);
// poseopt.hip keeps the same text in its kernel so far.  The
// quaternion algebra and Rodrigues underneath are
// lm_device.h's.  Everything is indexed at compile time, so a lane keeps its
// values in registers.
#pragma once

#include <hip/hip_runtime.h>

#include "lm_device.h"

namespace orbgpu {
namespace se3 {

// SE3Quat::normalizeRotation
__device__ inline void quat_normalize(double (&q)[4]) {
    if (q[3] < 0) {
        for (int i = 0; i < 4; ++i) q[i] = -q[i];
    }
    const double n = __dsqrt_rn(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}

// SE3Quat::exp(x) * (eq, et)  (se3quat.h:223-257, 104-110); the outputs may not alias the inputs
__device__ inline void se3_exp_times(const double (&eq)[4], const double (&et)[3], const double (&x)[6],
                                     double (&oq)[4], double (&ot)[3]) {
    double O[3][3], O2[3][3], R[9], V[3][3];
    const double theta = lm::rodrigues(x[0], x[1], x[2], O, O2, R);
    if (theta < lm::kSmallAngle) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) V[i][j] = R[3 * i + j];
    } else {
        const double sn = sin(theta), cs = cos(theta);
        const double b = (1.0 - cs) / (theta * theta);
        const double d = (theta - sn) / ((theta * theta) * theta);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) V[i][j] = ((i == j ? 1.0 : 0.0) + b * O[i][j]) + d * O2[i][j];
    }
    double te[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) te[i] = (V[i][0] * x[3] + V[i][1] * x[4]) + V[i][2] * x[5];
    double a[4];
    lm::quat_from_R(R, a);
    quat_normalize(a);
    // SE3Quat::operator*: t = ta + qa * tb, q = qa * qb, normalised
    double r0, r1, r2;
    lm::quat_rotate(a, et[0], et[1], et[2], r0, r1, r2);
    lm::quat_mul(a, eq, oq);
    quat_normalize(oq);
    ot[0] = te[0] + r0;
    ot[1] = te[1] + r1;
    ot[2] = te[2] + r2;
}

// Eigen's Quaternion::toRotationMatrix of q, not normalised, as lm::write_T16 has it
__device__ inline void quat_to_R(const double (&q)[4], double (&R)[3][3]) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0][0] = 1.0 - (tyy + tzz), R[0][1] = txy - twz, R[0][2] = txz + twy;
    R[1][0] = txy + twz, R[1][1] = 1.0 - (txx + tzz), R[1][2] = tyz - twx;
    R[2][0] = txz - twy, R[2][1] = tyz + twx, R[2][2] = 1.0 - (txx + tyy);
}

// Converter::toSE3Quat of a row-major 3x4 float [R | t]
__device__ inline void pose_from_T12(const float* T12, double (&q)[4], double (&t)[3]) {
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int col = 0; col < 3; ++col) R[3 * r + col] = (double)T12[4 * r + col];
    lm::quat_from_R(R, q);
    quat_normalize(q);
    for (int r = 0; r < 3; ++r) t[r] = (double)T12[4 * r + 3];
}

}  // namespace se3
}  // namespace orbgpu

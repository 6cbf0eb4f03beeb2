// projection_edge.h -- g2o's two binary projection edges, EdgeSE3ProjectXYZ and
// EdgeStereoSE3ProjectXYZ (types/types_six_dof_expmap.cpp:112-168, 199-245),
// over values in registers: computeError, which is the OnlyPose edges' too
// (:285-385), and linearizeOplus of both vertices, for localba.hip through
// ba_schur_device.h.  poseopt.hip and globalba.hip hold the same text in their
// kernels so far.  No memory access.
// -ffp-contract=off and the parentheses are what make the bits g2o's: the
// expressions are not to be rearranged.  The Huber thresholds of the callers
// are made here too, on the host, for all three files.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "lm_device.h"

namespace orbgpu {
namespace proj_edge {

struct Cam {
    double fx, fy, cx, cy, bf;
};

__device__ __forceinline__ Cam load_cam(const float* c) {
    return {(double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4]};
}

// Huber's delta = (float)sqrt(chi-square threshold) and its float square (dsqr), as doubles
struct HuberConst {
    double delta_mono, delta_stereo, dsqr_mono, dsqr_stereo;
};

inline HuberConst huber_constants(double chi2_mono, double chi2_stereo) {
    const float dm = (float)std::sqrt(chi2_mono), ds = (float)std::sqrt(chi2_stereo);
    // robust_kernel_impl.h:85: float dsqr = delta * delta (delta a double)
    return {(double)dm, (double)ds, (double)(float)((double)dm * (double)dm), (double)(float)((double)ds * (double)ds)};
}

// computeError at the pose (q, t) of the point X, observed at obs = (u, v, ur; ur < 0: monocular)
// with information w I: the camera-frame point (x, y, z), the error e and chi2 = e . (w e).
// invz = 1.0 / z is taken once, ahead of the branch: the stereo projection rounds it to float, the
// OnlyPose linearizeOplus of poseopt.hip uses it as it is.
__device__ __forceinline__ double project_error(const double (&q)[4], const double (&t)[3], const double (&X)[3],
                                                const Cam& cam, const float (&obs)[3], double w, double& x,
                                                double& y, double& z, double& invz, double (&e)[3]) {
    double r0, r1, r2;
    lm::quat_rotate(q, X[0], X[1], X[2], r0, r1, r2);
    x = r0 + t[0], y = r1 + t[1], z = r2 + t[2];
    invz = 1.0 / z;
    if (obs[2] >= 0.0f) {
        // const float invz = 1.0f / trans_xyz[2]: trans_xyz is a Vector3d, so the quotient is taken
        // in double and rounded to float once
        const double invzf = (double)(float)invz;
        const double us = (x * invzf) * cam.fx + cam.cx;
        const double vs = (y * invzf) * cam.fy + cam.cy;
        const double rs = us - cam.bf * invzf;
        e[0] = (double)obs[0] - us;
        e[1] = (double)obs[1] - vs;
        e[2] = (double)obs[2] - rs;
        return (e[0] * (w * e[0]) + e[1] * (w * e[1])) + e[2] * (w * e[2]);
    }
    e[0] = (double)obs[0] - ((x / z) * cam.fx + cam.cx);
    e[1] = (double)obs[1] - ((y / z) * cam.fy + cam.cy);
    e[2] = 0.0;
    return e[0] * (w * e[0]) + e[1] * (w * e[1]);
}

// linearizeOplus of the binary edges at the camera-frame point (x, y, z), R the pose's rotation:
// Jp (3 x 6) of the pose, Jl (3 x 3) of the point; a monocular edge's third rows are zero
__device__ __forceinline__ void linearize_xyz_se3(double x, double y, double z, const double (&R)[3][3],
                                                  const Cam& cam, bool stereo, double (&Jp)[3][6],
                                                  double (&Jl)[3][3]) {
    const double fx = cam.fx, fy = cam.fy, bf = cam.bf;
    const double z_2 = z * z;
    if (stereo) {
        for (int col = 0; col < 3; ++col) {
            Jl[0][col] = ((-fx) * R[0][col]) / z + ((fx * x) * R[2][col]) / z_2;
            Jl[1][col] = ((-fy) * R[1][col]) / z + ((fy * y) * R[2][col]) / z_2;
            Jl[2][col] = Jl[0][col] - (bf * R[2][col]) / z_2;
        }
    } else {  // -1./z * tmp * R
        const double s = -1.0 / z;
        const double t00 = s * fx, t01 = s * 0.0, t02 = s * (((-x) / z) * fx);
        const double t10 = s * 0.0, t11 = s * fy, t12 = s * (((-y) / z) * fy);
        for (int col = 0; col < 3; ++col) {
            Jl[0][col] = (t00 * R[0][col] + t01 * R[1][col]) + t02 * R[2][col];
            Jl[1][col] = (t10 * R[0][col] + t11 * R[1][col]) + t12 * R[2][col];
            Jl[2][col] = 0.0;
        }
    }
    Jp[0][0] = ((x * y) / z_2) * fx;
    Jp[0][1] = (-(1.0 + (x * x) / z_2)) * fx;
    Jp[0][2] = (y / z) * fx;
    Jp[0][3] = (-1.0 / z) * fx;
    Jp[0][4] = 0.0;
    Jp[0][5] = (x / z_2) * fx;
    Jp[1][0] = (1.0 + (y * y) / z_2) * fy;
    Jp[1][1] = (((-x) * y) / z_2) * fy;
    Jp[1][2] = ((-x) / z) * fy;
    Jp[1][3] = 0.0;
    Jp[1][4] = (-1.0 / z) * fy;
    Jp[1][5] = (y / z_2) * fy;
    if (stereo) {
        Jp[2][0] = Jp[0][0] - (bf * y) / z_2;
        Jp[2][1] = Jp[0][1] + (bf * x) / z_2;
        Jp[2][2] = Jp[0][2];
        Jp[2][3] = Jp[0][3];
        Jp[2][4] = 0.0;
        Jp[2][5] = Jp[0][5] - bf / z_2;
    } else {
        for (int k = 0; k < 6; ++k) Jp[2][k] = 0.0;
    }
}

}  // namespace proj_edge
}  // namespace orbgpu

// Sim3Optimizer.h -- Optimizer::OptimizeSim3 (reference:
// ORB-SLAM2/include/Optimizer.h:56-57, src/Optimizer.cpp:1229-1433; caller
// src/LoopClosing.cpp:393) on the MI355X through include/orbgpu_sim3opt.h.
// Header-only; link liborbgpu.so.
//
//   int ORB_SLAM2::OptimizeSim3GPU(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1,
//                                  g2o::Sim3& g2oS12, const float th2, const bool bFixScale, int device = -1)
//
// does what the reference's function does to its arguments: the gather of
// :1284-1366 (a correspondence is an index i with vpMatches1[i], a MapPoint of
// pKF1 at i, neither bad, and the match seen by pKF2), the two optimisations
// and checks on the device, vpMatches1[idx] = NULL where a check fails, g2oS12
// rewritten only when the second optimisation ran, nIn returned.  The class
// Optimizer is not replaced; the reference's member forwards here in one line
// (INTEGRATION.md §5c).  A template over the keyframe, MapPoint and Sim3 types:
// of the Sim3 type it uses rotation() (.x() .y() .z() .w()), translation()
// ([0..2]), scale() and the (Quaternion(w, x, y, z), Vector3(x, y, z), double)
// constructor, so g2o::Sim3 deduces and no Eigen header is needed here.
#ifndef ORBSLAM2_AMD_SIM3OPTIMIZER_H
#define ORBSLAM2_AMD_SIM3OPTIMIZER_H

#ifdef ORBGPU_CV_HEADER
#include ORBGPU_CV_HEADER
#else
#include <opencv2/core/core.hpp>
#endif

#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../orbgpu_sim3opt.h"
#include "Device.h"

namespace ORB_SLAM2 {

// device (adapter-only, Device.h): the GPU the call runs on (-1: the thread's)
template <class KeyFrameT, class MapPointT, class Sim3T>
int OptimizeSim3GPU(KeyFrameT* pKF1, KeyFrameT* pKF2, std::vector<MapPointT*>& vpMatches1, Sim3T& g2oS12,
                    const float th2, const bool bFixScale, int device = -1) {
    typedef typename std::decay<decltype(g2oS12.rotation())>::type QuatT;
    typedef typename std::decay<decltype(g2oS12.translation())>::type Vec3T;
    const cv::Mat& K1 = pKF1->mK;
    const cv::Mat& K2 = pKF2->mK;
    const cv::Mat R1w = pKF1->GetRotation();
    const cv::Mat t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation();
    const cv::Mat t2w = pKF2->GetTranslation();

    const int N = (int)vpMatches1.size();
    const std::vector<MapPointT*> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<float> P1c, P2c, obs1, obs2, w1, w2;
    std::vector<size_t> vnIndexEdge;
    for (int i = 0; i < N; ++i) {
        if (!vpMatches1[i]) continue;
        MapPointT* pMP1 = vpMapPoints1[i];
        MapPointT* pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;
        cv::Mat P3D1w = pMP1->GetWorldPos();
        cv::Mat P3D1c = R1w * P3D1w + t1w;
        cv::Mat P3D2w = pMP2->GetWorldPos();
        cv::Mat P3D2c = R2w * P3D2w + t2w;
        for (int k = 0; k < 3; ++k) {
            P1c.push_back(P3D1c.template at<float>(k));
            P2c.push_back(P3D2c.template at<float>(k));
        }
        const cv::KeyPoint& kpUn1 = pKF1->mvKeysUn[i];
        obs1.push_back(kpUn1.pt.x);
        obs1.push_back(kpUn1.pt.y);
        w1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
        const cv::KeyPoint& kpUn2 = pKF2->mvKeysUn[i2];
        obs2.push_back(kpUn2.pt.x);
        obs2.push_back(kpUn2.pt.y);
        w2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
        vnIndexEdge.push_back((size_t)i);
    }
    const int n = (int)vnIndexEdge.size();
    if (n == 0) return 0;  // nothing to optimise: no check fails, fewer than 10 correspondences

    orbgpu_sim3opt_job job;
    job.n = n;
    job.offset = 0;
    const QuatT& q = g2oS12.rotation();
    job.q12[0] = q.x(), job.q12[1] = q.y(), job.q12[2] = q.z(), job.q12[3] = q.w();
    for (int k = 0; k < 3; ++k) job.t12[k] = g2oS12.translation()[k];
    job.s12 = g2oS12.scale();
    job.K1[0] = K1.template at<float>(0, 0), job.K1[1] = K1.template at<float>(1, 1);
    job.K1[2] = K1.template at<float>(0, 2), job.K1[3] = K1.template at<float>(1, 2);
    job.K2[0] = K2.template at<float>(0, 0), job.K2[1] = K2.template at<float>(1, 1);
    job.K2[2] = K2.template at<float>(0, 2), job.K2[3] = K2.template at<float>(1, 2);
    job.th2 = th2;
    job.fix_scale = bFixScale ? 1 : 0;
    std::vector<uint8_t> removed((size_t)n, 0);
    orbgpu_sim3opt_result r;
    {
        const orbslam2_amd::DeviceGuard device_guard(device);
        if (orbgpu_optimize_sim3_batch(1, &job, n, P1c.data(), P2c.data(), obs1.data(), obs2.data(), w1.data(),
                                       w2.data(), &r, removed.data()) != ORBGPU_OK)
            throw std::runtime_error(std::string("orbgpu: ") + orbgpu_last_error());
    }
    for (int k = 0; k < n; ++k)
        if (removed[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPointT*>(NULL);
    if (r.rounds < 2) return 0;  // Optimizer.cpp:1402-1403: g2oS12 is not written
    g2oS12 = Sim3T(QuatT(r.q12[3], r.q12[0], r.q12[1], r.q12[2]), Vec3T(r.t12[0], r.t12[1], r.t12[2]), r.s12);
    return r.n_in;
}

}  // namespace ORB_SLAM2

#endif

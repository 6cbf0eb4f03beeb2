// PoseOptimizer.h -- Optimizer::PoseOptimization (reference:
// ORB-SLAM2/include/Optimizer.h:53, src/Optimizer.cpp:291-513) on the MI355X
// through include/orbgpu_poseopt.h.  Header-only; link liborbgpu.so.
//
//   int ORB_SLAM2::PoseOptimizationGPU(Frame* pFrame, int device = -1)
//
// does what the reference's function does to the frame: every keypoint with a
// MapPoint becomes a monocular (mvuRight < 0) or stereo edge, mvbOutlier of
// those keypoints is rewritten, the optimised pose goes through SetPose and the
// return value is nInitialCorrespondences - nBad.  The class Optimizer is not
// replaced -- its bundle-adjustment members stay with g2o; the reference's
// Optimizer::PoseOptimization forwards here in one line.
// A template over the frame type, so the reference's Frame deduces.
#ifndef ORBSLAM2_AMD_POSEOPTIMIZER_H
#define ORBSLAM2_AMD_POSEOPTIMIZER_H

#ifdef ORBGPU_CV_HEADER
#include ORBGPU_CV_HEADER
#else
#include <opencv2/core/core.hpp>
#endif

#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../orbgpu_poseopt.h"
#include "Device.h"

namespace ORB_SLAM2 {

// device (adapter-only, Device.h): the GPU the call runs on (-1: the thread's)
template <class FrameT>
int PoseOptimizationGPU(FrameT* pFrame, int device = -1) {
    typedef typename std::remove_pointer<
        typename std::remove_reference<decltype(pFrame->mvpMapPoints)>::type::value_type>::type MapPointT;
    const int N = pFrame->N;
    std::vector<float> Xw, obs, inv_sigma2;
    std::vector<int> index;  // keypoint of each observation
    {
        // Optimizer.cpp:335-420: the MapPoint positions are read under the global mutex
        std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
        for (int i = 0; i < N; ++i) {
            MapPointT* pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            const cv::KeyPoint& kpUn = pFrame->mvKeysUn[i];
            const cv::Mat Pos = pMP->GetWorldPos();
            for (int k = 0; k < 3; ++k) Xw.push_back(Pos.template at<float>(k));
            obs.push_back(kpUn.pt.x);
            obs.push_back(kpUn.pt.y);
            obs.push_back(pFrame->mvuRight[i]);
            inv_sigma2.push_back(pFrame->mvInvLevelSigma2[kpUn.octave]);
            index.push_back(i);
        }
    }
    const int n = (int)index.size();
    orbgpu_poseopt_job job;
    job.n = n;
    job.offset = 0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) job.Tcw0[4 * r + c] = pFrame->mTcw.template at<float>(r, c);
    job.fx = pFrame->fx;
    job.fy = pFrame->fy;
    job.cx = pFrame->cx;
    job.cy = pFrame->cy;
    job.bf = pFrame->mbf;
    job.pad = 0;
    std::vector<uint8_t> outlier(n > 0 ? n : 1, 0);
    orbgpu_poseopt_result r;
    {
        const orbslam2_amd::DeviceGuard device_guard(device);
        if (orbgpu_pose_optimization_batch(1, &job, n, Xw.data(), obs.data(), inv_sigma2.data(), &r,
                                           outlier.data()) != ORBGPU_OK)
            throw std::runtime_error(std::string("orbgpu: ") + orbgpu_last_error());
    }
    // mvbOutlier only at keypoints with a MapPoint (Optimizer.cpp:348, :382, :459-465)
    for (int k = 0; k < n; ++k) pFrame->mvbOutlier[index[k]] = outlier[k] != 0;
    if (n < 3) return 0;  // Optimizer.cpp:423-424: the pose is not touched
    cv::Mat pose(4, 4, CV_32F);
    for (int rr = 0; rr < 4; ++rr)
        for (int c = 0; c < 4; ++c) pose.at<float>(rr, c) = r.Tcw[4 * rr + c];
    pFrame->SetPose(pose);
    return r.n_good;
}

}  // namespace ORB_SLAM2

#endif

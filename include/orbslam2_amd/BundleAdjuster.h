// BundleAdjuster.h -- Optimizer::BundleAdjustment and
// Optimizer::GlobalBundleAdjustemnt (reference: ORB-SLAM2/include/Optimizer.h,
// src/Optimizer.cpp:44-269; callers Tracking::CreateInitialMapMonocular,
// src/Tracking.cpp:887, and LoopClosing::RunGlobalBundleAdjustment,
// src/LoopClosing.cpp:782) on the MI355X through include/orbgpu_globalba.h.
// Header-only; link liborbgpu.so.
//
//   void ORB_SLAM2::BundleAdjustmentGPU(vpKFs, vpMP, nIterations = 5, pbStopFlag = NULL, nLoopKF = 0,
//                                       bRobust = true, device = -1)
//   void ORB_SLAM2::GlobalBundleAdjustemntGPU(pMap, nIterations = 5, pbStopFlag = NULL, nLoopKF = 0,
//                                             bRobust = true, device = -1)      (the reference's spelling)
//
// do what the reference's functions do to their arguments: the gather of :98-214
// in the reference's order (a pose per keyframe that is not bad, fixed for mnId
// == 0, and maxKFid over them; a point per MapPoint that is not bad; an edge per
// observation by a keyframe that is not bad and whose mnId is at most maxKFid,
// in GetObservations() order; a MapPoint left without an edge is "not included"
// and not written back), one optimize(nIterations) on the device with Huber on
// every edge iff bRobust, then the write-back of :225-267: SetPose and
// SetWorldPos + UpdateNormalAndDepth when nLoopKF == 0, otherwise mTcwGBA,
// mPosGBA and mnBAGlobalForKF = nLoopKF.  pbStopFlag is passed through: the
// optimisation polls it where g2o does.  An observation by a keyframe that is
// not among vpKFs makes no edge (the reference would hand g2o a null vertex).
// The class Optimizer is not replaced; the reference's members forward here in
// one line.  Templates over the keyframe, MapPoint and map
// types.
#ifndef ORBSLAM2_AMD_BUNDLEADJUSTER_H
#define ORBSLAM2_AMD_BUNDLEADJUSTER_H

#ifdef ORBGPU_CV_HEADER
#include ORBGPU_CV_HEADER
#else
#include <opencv2/core/core.hpp>
#endif

#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../orbgpu_globalba.h"
#include "Device.h"

namespace ORB_SLAM2 {

// device (adapter-only, Device.h): the GPU the call runs on (-1: the thread's)
template <class KeyFrameT, class MapPointT>
void BundleAdjustmentGPU(const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMP, int nIterations = 5,
                         bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0, const bool bRobust = true,
                         int device = -1) {
    static_assert(sizeof(bool) == 1, "the stop flag is read as one byte");
    std::vector<bool> vbNotIncludedMP;
    vbNotIncludedMP.resize(vpMP.size());

    long unsigned int maxKFid = 0;

    // Set KeyFrame vertices
    std::map<KeyFrameT*, int> pose_index;
    std::vector<float> Tcw, cam;
    std::vector<uint8_t> fixed;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrameT* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        pose_index[pKF] = (int)fixed.size();
        const cv::Mat T = pKF->GetPose();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) Tcw.push_back(T.template at<float>(r, c));
        fixed.push_back(pKF->mnId == 0 ? 1 : 0);
        const float k[5] = {pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf};
        cam.insert(cam.end(), k, k + 5);
        if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
    }

    // Set MapPoint vertices and the edges, grouped by point
    std::vector<float> Xw, obs, inv_sigma2;
    std::vector<int> edge_pose, edge_point, point_index(vpMP.size(), -1);
    for (size_t i = 0; i < vpMP.size(); i++) {
        MapPointT* pMP = vpMP[i];
        if (pMP->isBad()) continue;
        const int m = (int)(Xw.size() / 3);
        point_index[i] = m;
        const cv::Mat pos = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) Xw.push_back(pos.template at<float>(k));
        const std::map<KeyFrameT*, size_t> observations = pMP->GetObservations();
        int nEdges = 0;
        for (typename std::map<KeyFrameT*, size_t>::const_iterator mit = observations.begin();
             mit != observations.end(); mit++) {
            KeyFrameT* pKF = mit->first;
            if (pKF->isBad() || pKF->mnId > maxKFid) continue;
            const typename std::map<KeyFrameT*, int>::const_iterator where = pose_index.find(pKF);
            if (where == pose_index.end()) continue;
            nEdges++;
            const cv::KeyPoint& kpUn = pKF->mvKeysUn[mit->second];
            const float kp_ur = pKF->mvuRight[mit->second];
            obs.push_back(kpUn.pt.x);
            obs.push_back(kpUn.pt.y);
            obs.push_back(kp_ur < 0 ? -1.0f : kp_ur);
            inv_sigma2.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
            edge_pose.push_back(where->second);
            edge_point.push_back(m);
        }
        vbNotIncludedMP[i] = nEdges == 0;
    }

    // Optimize!
    const int n_poses = (int)fixed.size(), n_points = (int)(Xw.size() / 3), n_edges = (int)edge_pose.size();
    std::vector<float> Tcw_out((size_t)16 * n_poses), Xw_out((size_t)3 * n_points);
    if (n_poses + n_points > 0) {
        orbgpu_ba_result r;
        const orbslam2_amd::DeviceGuard device_guard(device);
        if (orbgpu_bundle_adjustment(n_poses, n_points, n_edges, Tcw.data(), fixed.data(), cam.data(), Xw.data(),
                                     edge_pose.data(), edge_point.data(), obs.data(), inv_sigma2.data(), nIterations,
                                     bRobust ? 1 : 0, reinterpret_cast<const volatile uint8_t*>(pbStopFlag),
                                     Tcw_out.data(), Xw_out.data(), &r, NULL, 0) != ORBGPU_OK)
            throw std::runtime_error(std::string("orbgpu: ") + orbgpu_last_error());
    }

    // Recover optimized data: keyframes, then points
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrameT* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const typename std::map<KeyFrameT*, int>::const_iterator where = pose_index.find(pKF);
        if (where == pose_index.end()) continue;  // it turned good since the gather
        cv::Mat T(4, 4, CV_32F);
        for (int e = 0; e < 16; ++e) T.template at<float>(e / 4, e % 4) = Tcw_out[(size_t)16 * where->second + e];
        if (nLoopKF == 0) {
            pKF->SetPose(T);
        } else {
            pKF->mTcwGBA = T;
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    for (size_t i = 0; i < vpMP.size(); i++) {
        if (vbNotIncludedMP[i]) continue;
        MapPointT* pMP = vpMP[i];
        if (pMP->isBad() || point_index[i] < 0) continue;
        cv::Mat pos(3, 1, CV_32F);
        for (int e = 0; e < 3; ++e) pos.template at<float>(e) = Xw_out[(size_t)3 * point_index[i] + e];
        if (nLoopKF == 0) {
            pMP->SetWorldPos(pos);
            pMP->UpdateNormalAndDepth();
        } else {
            pMP->mPosGBA = pos;
            pMP->mnBAGlobalForKF = nLoopKF;
        }
    }
}

template <class MapT>
void GlobalBundleAdjustemntGPU(MapT* pMap, int nIterations = 5, bool* pbStopFlag = NULL, const unsigned long nLoopKF = 0,
                               const bool bRobust = true, int device = -1) {
    BundleAdjustmentGPU(pMap->GetAllKeyFrames(), pMap->GetAllMapPoints(), nIterations, pbStopFlag, nLoopKF, bRobust,
                        device);
}

}  // namespace ORB_SLAM2

#endif

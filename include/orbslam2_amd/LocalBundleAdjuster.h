// LocalBundleAdjuster.h -- Optimizer::LocalBundleAdjustment (reference:
// ORB-SLAM2/include/Optimizer.h, src/Optimizer.cpp:536-885; caller
// src/LocalMapping.cpp, LocalMapping::Run) on the MI355X through
// include/orbgpu_localba.h.  Header-only; link liborbgpu.so.
//
//   void ORB_SLAM2::LocalBundleAdjustmentGPU(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int device = -1)
//   void ORB_SLAM2::LocalBundleAdjustmentChipGPU(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int device = -1)
//
// The first does what the reference's function does to its arguments: the gather of
// :540-752 in the reference's order with its mnBALocalForKF / mnBAFixedForKF
// bookkeeping (local keyframes: pKF, then its covisible keyframes that are not
// bad; local MapPoints: those of the local keyframes, not bad, first seen first;
// fixed keyframes: the other observers of those points, not bad; one edge per
// observation by a keyframe that is not bad, in GetObservations() order), the
// two optimisations on the device, then under pMap->mMutexMapUpdate the
// erasures in the reference's order (monocular edges, then stereo), SetPose of
// every local keyframe and SetWorldPos + UpdateNormalAndDepth of every local
// MapPoint.  *pbStopFlag is read once, before the call (:754-756); g2o's
// mid-run stop is not reproduced by the first form (one asynchronous launch per
// batch); the second, through include/orbgpu_localba_chip.h, spreads the one
// neighbourhood over the whole chip and hands pbStopFlag to a host loop that
// polls it where g2o does and reads it between the rounds (:764-766).  Both share
// the gather, the erasure replay and the write-back (localba_detail).  Neither
// reproduces a MapPoint that turns bad
// while the optimisation runs (the reference skips its edge in the first
// classification).  The class Optimizer is not replaced; the reference's member
// forwards here in one line.  A template over the keyframe
// and map types; the MapPoint type is the one GetMapPointMatches() holds.
#ifndef ORBSLAM2_AMD_LOCALBUNDLEADJUSTER_H
#define ORBSLAM2_AMD_LOCALBUNDLEADJUSTER_H

#ifdef ORBGPU_CV_HEADER
#include ORBGPU_CV_HEADER
#else
#include <opencv2/core/core.hpp>
#endif

#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../orbgpu_localba.h"
#include "../orbgpu_localba_chip.h"
#include "Device.h"

namespace ORB_SLAM2 {

namespace localba_detail {

// what the gather of :540-752 leaves: the lists, and the job's arrays in orbgpu_localba.h's layout
template <class KeyFrameT, class MapPointT>
struct Gathered {
    std::list<KeyFrameT*> lLocalKeyFrames, lFixedCameras;
    std::list<MapPointT*> lLocalMapPoints;
    std::vector<float> Tcw, cam, Xw, obs, inv_sigma2;
    std::vector<uint8_t> fixed;
    std::vector<int> edge_pose, edge_point;
    std::vector<KeyFrameT*> vpEdgeKF;
    std::vector<MapPointT*> vpMapPointEdge;
    int n_local() const { return (int)lLocalKeyFrames.size(); }
    int n_poses() const { return (int)fixed.size(); }
    int n_points() const { return (int)lLocalMapPoints.size(); }
    int n_edges() const { return (int)edge_pose.size(); }
};

template <class KeyFrameT, class MapPointT>
void Gather(KeyFrameT* pKF, Gathered<KeyFrameT, MapPointT>& g) {
    typedef typename std::decay<decltype(pKF->GetMapPointMatches())>::type MapPointVecT;
    std::list<KeyFrameT*>&lLocalKeyFrames = g.lLocalKeyFrames, &lFixedCameras = g.lFixedCameras;
    std::list<MapPointT*>& lLocalMapPoints = g.lLocalMapPoints;
    std::vector<float>&Tcw = g.Tcw, &cam = g.cam, &Xw = g.Xw, &obs = g.obs, &inv_sigma2 = g.inv_sigma2;
    std::vector<uint8_t>& fixed = g.fixed;
    std::vector<int>&edge_pose = g.edge_pose, &edge_point = g.edge_point;
    std::vector<KeyFrameT*>& vpEdgeKF = g.vpEdgeKF;
    std::vector<MapPointT*>& vpMapPointEdge = g.vpMapPointEdge;

    // Local KeyFrames: First Breadth Search from Current Keyframe
    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    const std::vector<KeyFrameT*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = (int)vNeighKFs.size(); i < iend; i++) {
        KeyFrameT* pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }

    // Local MapPoints seen in Local KeyFrames
    for (typename std::list<KeyFrameT*>::iterator lit = lLocalKeyFrames.begin(); lit != lLocalKeyFrames.end(); lit++) {
        MapPointVecT vpMPs = (*lit)->GetMapPointMatches();
        for (typename MapPointVecT::iterator vit = vpMPs.begin(); vit != vpMPs.end(); vit++) {
            MapPointT* pMP = *vit;
            if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
                lLocalMapPoints.push_back(pMP);
                pMP->mnBALocalForKF = pKF->mnId;
            }
        }
    }

    // Fixed Keyframes. Keyframes that see Local MapPoints but that are not Local Keyframes
    for (typename std::list<MapPointT*>::iterator lit = lLocalMapPoints.begin(); lit != lLocalMapPoints.end(); lit++) {
        std::map<KeyFrameT*, size_t> observations = (*lit)->GetObservations();
        for (typename std::map<KeyFrameT*, size_t>::iterator mit = observations.begin(); mit != observations.end();
             mit++) {
            KeyFrameT* pKFi = mit->first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    }

    // the vertices: local poses, fixed poses, points
    std::map<KeyFrameT*, int> pose_index;
    for (int pass = 0; pass < 2; ++pass) {
        std::list<KeyFrameT*>& l = pass == 0 ? lLocalKeyFrames : lFixedCameras;
        for (typename std::list<KeyFrameT*>::iterator lit = l.begin(); lit != l.end(); lit++) {
            KeyFrameT* pKFi = *lit;
            pose_index[pKFi] = (int)fixed.size();
            const cv::Mat T = pKFi->GetPose();
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) Tcw.push_back(T.template at<float>(r, c));
            fixed.push_back(pass == 1 || pKFi->mnId == 0 ? 1 : 0);
            const float k[5] = {pKFi->fx, pKFi->fy, pKFi->cx, pKFi->cy, pKFi->mbf};
            cam.insert(cam.end(), k, k + 5);
        }
    }
    // the edges, grouped by point
    int m = 0;
    for (typename std::list<MapPointT*>::iterator lit = lLocalMapPoints.begin(); lit != lLocalMapPoints.end();
         lit++, ++m) {
        MapPointT* pMP = *lit;
        const cv::Mat pos = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) Xw.push_back(pos.template at<float>(k));
        const std::map<KeyFrameT*, size_t> observations = pMP->GetObservations();
        for (typename std::map<KeyFrameT*, size_t>::const_iterator mit = observations.begin();
             mit != observations.end(); mit++) {
            KeyFrameT* pKFi = mit->first;
            if (pKFi->isBad()) continue;
            const typename std::map<KeyFrameT*, int>::const_iterator where = pose_index.find(pKFi);
            if (where == pose_index.end()) continue;  // it turned good since the lists were made
            const cv::KeyPoint& kpUn = pKFi->mvKeysUn[mit->second];
            const float kp_ur = pKFi->mvuRight[mit->second];
            obs.push_back(kpUn.pt.x);
            obs.push_back(kpUn.pt.y);
            obs.push_back(kp_ur < 0 ? -1.0f : kp_ur);
            inv_sigma2.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
            edge_pose.push_back(where->second);
            edge_point.push_back(m);
            vpEdgeKF.push_back(pKFi);
            vpMapPointEdge.push_back(pMP);
        }
    }

}

// the erasure replay of :779-803 / :823-847 and the write-back of :850-885 under pMap->mMutexMapUpdate
template <class KeyFrameT, class MapPointT, class MapT>
void WriteBack(Gathered<KeyFrameT, MapPointT>& g, MapT* pMap, const std::vector<float>& Tcw_out,
               const std::vector<float>& Xw_out, const std::vector<uint8_t>& erase) {
    std::list<KeyFrameT*>& lLocalKeyFrames = g.lLocalKeyFrames;
    std::list<MapPointT*>& lLocalMapPoints = g.lLocalMapPoints;
    const std::vector<float>& obs = g.obs;
    const std::vector<KeyFrameT*>& vpEdgeKF = g.vpEdgeKF;
    const std::vector<MapPointT*>& vpMapPointEdge = g.vpMapPointEdge;
    const int n_edges = g.n_edges();

    // vToErase: the monocular edges in edge order, then the stereo edges
    std::vector<std::pair<KeyFrameT*, MapPointT*> > vToErase;
    vToErase.reserve((size_t)n_edges);
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n_edges; ++i) {
            const bool stereo = !(obs[3 * (size_t)i + 2] < 0);
            if (stereo != (pass == 1) || !erase[i]) continue;
            if (vpMapPointEdge[i]->isBad()) continue;
            vToErase.push_back(std::make_pair(vpEdgeKF[i], vpMapPointEdge[i]));
        }

    // Get Map Mutex
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (size_t i = 0; i < vToErase.size(); i++) {
        KeyFrameT* pKFi = vToErase[i].first;
        MapPointT* pMPi = vToErase[i].second;
        pKFi->EraseMapPointMatch(pMPi);
        pMPi->EraseObservation(pKFi);
    }
    // Recover optimized data: keyframes, then points
    int k = 0;
    for (typename std::list<KeyFrameT*>::iterator lit = lLocalKeyFrames.begin(); lit != lLocalKeyFrames.end();
         lit++, ++k) {
        cv::Mat T(4, 4, CV_32F);
        for (int e = 0; e < 16; ++e) T.template at<float>(e / 4, e % 4) = Tcw_out[(size_t)16 * k + e];
        (*lit)->SetPose(T);
    }
    int m = 0;
    for (typename std::list<MapPointT*>::iterator lit = lLocalMapPoints.begin(); lit != lLocalMapPoints.end();
         lit++, ++m) {
        cv::Mat pos(3, 1, CV_32F);
        for (int e = 0; e < 3; ++e) pos.template at<float>(e) = Xw_out[(size_t)3 * m + e];
        (*lit)->SetWorldPos(pos);
        (*lit)->UpdateNormalAndDepth();
    }
}


}  // namespace localba_detail

// device (adapter-only, Device.h): the GPU the call runs on (-1: the thread's)
template <class KeyFrameT, class MapT>
void LocalBundleAdjustmentGPU(KeyFrameT* pKF, bool* pbStopFlag, MapT* pMap, int device = -1) {
    typedef typename std::decay<decltype(pKF->GetMapPointMatches())>::type MapPointVecT;
    typedef typename std::remove_pointer<typename MapPointVecT::value_type>::type MapPointT;
    localba_detail::Gathered<KeyFrameT, MapPointT> g;
    localba_detail::Gather(pKF, g);

    if (pbStopFlag)
        if (*pbStopFlag) return;

    const int n_local = g.n_local(), n_poses = g.n_poses(), n_points = g.n_points(), n_edges = g.n_edges();
    // no local MapPoint: nothing to optimise, and no device is needed.  (The reference would still
    // rewrite every local pose with its quaternion round trip; that is not reproduced.)
    if (n_points == 0) return;
    orbgpu_localba_job job;
    job.n_poses = n_poses, job.n_local = n_local, job.n_points = n_points, job.n_edges = n_edges;
    job.pose_offset = 0, job.point_offset = 0, job.edge_offset = 0, job.out_pose_offset = 0;
    std::vector<float> Tcw_out((size_t)16 * n_local), Xw_out((size_t)3 * n_points);
    std::vector<uint8_t> erase((size_t)n_edges, 0);
    orbgpu_localba_result r;
    {
        const orbslam2_amd::DeviceGuard device_guard(device);
        if (orbgpu_local_ba_batch(1, &job, n_poses, n_local, n_points, n_edges, n_local, g.Tcw.data(), g.fixed.data(),
                                  g.cam.data(), g.Xw.data(), g.edge_pose.data(), g.edge_point.data(), g.obs.data(),
                                  g.inv_sigma2.data(), Tcw_out.data(), Xw_out.data(), erase.data(), &r, NULL,
                                  0) != ORBGPU_OK)
            throw std::runtime_error(std::string("orbgpu: ") + orbgpu_last_error());
    }
    localba_detail::WriteBack(g, pMap, Tcw_out, Xw_out, erase);
}

// The same through include/orbgpu_localba_chip.h: the neighbourhood spread over the whole chip, and
// pbStopFlag passed through as the byte g2o's force-stop flag is, polled where g2o polls it and read
// between the rounds (:764-766).  It returns at :754-756 when the flag is already set.
template <class KeyFrameT, class MapT>
void LocalBundleAdjustmentChipGPU(KeyFrameT* pKF, bool* pbStopFlag, MapT* pMap, int device = -1) {
    static_assert(sizeof(bool) == 1, "the stop flag is read as one byte");
    typedef typename std::decay<decltype(pKF->GetMapPointMatches())>::type MapPointVecT;
    typedef typename std::remove_pointer<typename MapPointVecT::value_type>::type MapPointT;
    localba_detail::Gathered<KeyFrameT, MapPointT> g;
    localba_detail::Gather(pKF, g);

    if (pbStopFlag)
        if (*pbStopFlag) return;

    const int n_local = g.n_local(), n_poses = g.n_poses(), n_points = g.n_points(), n_edges = g.n_edges();
    if (n_points == 0) return;  // as above
    std::vector<float> Tcw_out((size_t)16 * n_local), Xw_out((size_t)3 * n_points);
    std::vector<uint8_t> erase((size_t)n_edges, 0);
    orbgpu_localba_chip_result r;
    {
        const orbslam2_amd::DeviceGuard device_guard(device);
        if (orbgpu_local_ba_chip(n_poses, n_local, n_points, n_edges, g.Tcw.data(), g.fixed.data(), g.cam.data(),
                                 g.Xw.data(), g.edge_pose.data(), g.edge_point.data(), g.obs.data(),
                                 g.inv_sigma2.data(), 5, 10, reinterpret_cast<const volatile uint8_t*>(pbStopFlag), -1,
                                 Tcw_out.data(), Xw_out.data(), erase.data(), &r, NULL, 0) != ORBGPU_OK)
            throw std::runtime_error(std::string("orbgpu: ") + orbgpu_last_error());
    }
    localba_detail::WriteBack(g, pMap, Tcw_out, Xw_out, erase);
}

}  // namespace ORB_SLAM2

#endif

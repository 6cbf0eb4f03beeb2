// EssentialGraphOptimizer.h -- Optimizer::OptimizeEssentialGraph (reference:
// ORB-SLAM2/include/Optimizer.h, src/Optimizer.cpp:905-1200; caller
// LoopClosing::CorrectLoop, src/LoopClosing.cpp:690) on the MI355X through
// include/orbgpu_essential.h.  Header-only; link liborbgpu.so.
//
//   void ORB_SLAM2::OptimizeEssentialGraphGPU(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3,
//                                             LoopConnections, bFixScale, nIterations = 20, device = -1)
//
// does what the reference's function does to its arguments:
//   vertices   every keyframe of GetAllKeyFrames() that is not bad, in that order, indexed densely;
//              its corrected and non-corrected Sim3 where the two maps have one; fixed for pLoopKF
//   edges      enumerated exactly as :989-1133: LoopConnections in map / set order with the
//              GetWeight < 100 skip and its pCurKF / pLoopKF exception (kind 0, and the pair enters
//              sInsertedEdges); then per keyframe of GetAllKeyFrames() the parent, the loop edges
//              with a smaller mnId, and GetCovisiblesByWeight(100) without the parent, the children,
//              the loop edges, bad keyframes, larger mnIds and pairs in sInsertedEdges (kind 1)
//   optimise   one call of orbgpu_optimize_essential_graph: optimize(nIterations), the SE3 recovery
//              and the MapPoint correction
//   write-back under unique_lock<mutex>(pMap->mMutexMapUpdate): SetPose per keyframe; per MapPoint that
//              is not bad SetWorldPos, then UpdateNormalAndDepth()
// A MapPoint's reference is mnCorrectedReference when mnCorrectedByKF == pCurKF->mnId, else
// GetReferenceKeyFrame()->mnId, mapped to the dense index; when that keyframe is not a vertex the point
// keeps its position (the reference reads a default-constructed identity Sim3 twice, which computes
// the same).
// Where this differs from the reference: an edge with an endpoint that is not a vertex (a bad
// keyframe, or one that is not in the map) is dropped, where the reference would hand g2o a null
// vertex; a bad keyframe gets no SetPose, where the reference dereferences a null vertex; the MapPoint
// positions are read before the optimisation, not under the lock after it.
// The class Optimizer is not replaced; the reference's member forwards here in one line
// (INTEGRATION.md §5i).  A template over the map, keyframe and container types: of the Sim3 type it
// uses only rotation() (.x() .y() .z() .w()), translation() ([0..2]) and scale(), so g2o::Sim3 deduces
// and no Eigen header is needed here.
#ifndef ORBSLAM2_AMD_ESSENTIALGRAPHOPTIMIZER_H
#define ORBSLAM2_AMD_ESSENTIALGRAPHOPTIMIZER_H

#ifdef ORBGPU_CV_HEADER
#include ORBGPU_CV_HEADER
#else
#include <opencv2/core/core.hpp>
#endif

#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../orbgpu_essential.h"
#include "Device.h"

namespace ORB_SLAM2 {

namespace essential_detail {
template <class Sim3T>
inline void sim3_to_row(const Sim3T& S, double* row) {
    row[0] = S.rotation().x(), row[1] = S.rotation().y(), row[2] = S.rotation().z(), row[3] = S.rotation().w();
    for (int k = 0; k < 3; ++k) row[4 + k] = S.translation()[k];
    row[7] = S.scale();
}
}  // namespace essential_detail

// nIterations, device (adapter-only; Device.h): optimize(20) in the reference; the GPU the call runs on
// (-1: the thread's)
template <class MapT, class KeyFrameT, class KeyFrameAndPoseT, class LoopConnectionsT>
void OptimizeEssentialGraphGPU(MapT* pMap, KeyFrameT* pLoopKF, KeyFrameT* pCurKF,
                               const KeyFrameAndPoseT& NonCorrectedSim3, const KeyFrameAndPoseT& CorrectedSim3,
                               const LoopConnectionsT& LoopConnections, const bool& bFixScale, int nIterations = 20,
                               int device = -1) {
    const std::vector<KeyFrameT*> vpKFs = pMap->GetAllKeyFrames();
    const auto vpMPs = pMap->GetAllMapPoints();

    const int minFeat = 100;

    // Set KeyFrame vertices
    std::map<KeyFrameT*, int> vertex_of;
    std::map<long unsigned int, int> vertex_of_id;
    std::vector<KeyFrameT*> vertices;
    std::vector<float> Tcw;
    std::vector<uint8_t> has_corrected, has_noncorrected, fixed;
    std::vector<double> Scorrected, Snoncorrected;
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrameT* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int v = (int)vertices.size();
        vertex_of[pKF] = v;
        vertex_of_id[pKF->mnId] = v;
        vertices.push_back(pKF);
        const cv::Mat T = pKF->GetPose();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) Tcw.push_back(T.template at<float>(r, c));
        double row[8] = {0, 0, 0, 1, 0, 0, 0, 1};
        const typename KeyFrameAndPoseT::const_iterator it = CorrectedSim3.find(pKF);
        has_corrected.push_back(it != CorrectedSim3.end() ? 1 : 0);
        if (it != CorrectedSim3.end()) essential_detail::sim3_to_row(it->second, row);
        Scorrected.insert(Scorrected.end(), row, row + 8);
        double nrow[8] = {0, 0, 0, 1, 0, 0, 0, 1};
        const typename KeyFrameAndPoseT::const_iterator itn = NonCorrectedSim3.find(pKF);
        has_noncorrected.push_back(itn != NonCorrectedSim3.end() ? 1 : 0);
        if (itn != NonCorrectedSim3.end()) essential_detail::sim3_to_row(itn->second, nrow);
        Snoncorrected.insert(Snoncorrected.end(), nrow, nrow + 8);
        fixed.push_back(pKF == pLoopKF ? 1 : 0);
    }

    std::vector<int> edge_i, edge_j;
    std::vector<uint8_t> edge_kind;
    const auto add_edge = [&](KeyFrameT* pKFi, KeyFrameT* pKFj, uint8_t kind) {
        const typename std::map<KeyFrameT*, int>::const_iterator wi = vertex_of.find(pKFi), wj = vertex_of.find(pKFj);
        if (wi == vertex_of.end() || wj == vertex_of.end() || wi->second == wj->second) return;
        edge_i.push_back(wi->second), edge_j.push_back(wj->second), edge_kind.push_back(kind);
    };

    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;

    // Set Loop edges
    for (typename LoopConnectionsT::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end();
         mit != mend; mit++) {
        KeyFrameT* pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const auto& spConnections = mit->second;
        for (auto sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            add_edge(pKF, *sit, 0);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }

    // Set normal edges
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        KeyFrameT* pKF = vpKFs[i];
        KeyFrameT* pParentKF = pKF->GetParent();

        // Spanning tree edge
        if (pParentKF) add_edge(pKF, pParentKF, 1);

        // Loop edges
        const std::set<KeyFrameT*> sLoopEdges = pKF->GetLoopEdges();
        for (typename std::set<KeyFrameT*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end();
             sit != send; sit++) {
            KeyFrameT* pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) add_edge(pKF, pLKF, 1);
        }

        // Covisibility graph edges
        const std::vector<KeyFrameT*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (typename std::vector<KeyFrameT*>::const_iterator vit = vpConnectedKFs.begin();
             vit != vpConnectedKFs.end(); vit++) {
            KeyFrameT* pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId),
                                                            std::max(pKF->mnId, pKFn->mnId))))
                        continue;
                    add_edge(pKF, pKFn, 1);
                }
            }
        }
    }

    // MapPoints: the position and the reference keyframe's vertex
    std::vector<float> Xw;
    std::vector<int> point_ref, point_index(vpMPs.size(), -1);
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        auto* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        long unsigned int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) {
            nIDr = pMP->mnCorrectedReference;
        } else {
            KeyFrameT* pRefKF = pMP->GetReferenceKeyFrame();
            nIDr = pRefKF->mnId;
        }
        const std::map<long unsigned int, int>::const_iterator where = vertex_of_id.find(nIDr);
        point_index[i] = (int)point_ref.size();
        point_ref.push_back(where == vertex_of_id.end() ? -1 : where->second);
        const cv::Mat P3Dw = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) Xw.push_back(P3Dw.template at<float>(k));
    }

    // Optimize!
    const int n_kf = (int)vertices.size(), n_edges = (int)edge_i.size(), n_points = (int)point_ref.size();
    std::vector<double> Scw_out((size_t)8 * n_kf);
    std::vector<float> Tcw_out((size_t)16 * n_kf), Xw_out((size_t)3 * n_points);
    if (n_kf + n_points > 0) {
        orbgpu_eg_result r;
        const orbslam2_amd::DeviceGuard device_guard(device);
        if (orbgpu_optimize_essential_graph(n_kf, n_edges, n_points, Tcw.data(), has_corrected.data(), Scorrected.data(),
                                            has_noncorrected.data(), Snoncorrected.data(), fixed.data(), edge_i.data(),
                                            edge_j.data(), edge_kind.data(), Xw.data(), point_ref.data(),
                                            bFixScale ? 1 : 0, nIterations, Scw_out.data(), Tcw_out.data(),
                                            Xw_out.data(), &r, NULL, 0) != ORBGPU_OK)
            throw std::runtime_error(std::string("orbgpu: ") + orbgpu_last_error());
    }

    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);

    // SE3 Pose Recovering. Sim3:[sR t;0 1] -> SE3:[R t/s;0 1]
    for (int v = 0; v < n_kf; ++v) {
        cv::Mat Tiw(4, 4, CV_32F);
        for (int e = 0; e < 16; ++e) Tiw.template at<float>(e / 4, e % 4) = Tcw_out[(size_t)16 * v + e];
        vertices[v]->SetPose(Tiw);
    }

    // Correct points
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
        auto* pMP = vpMPs[i];
        if (point_index[i] < 0 || pMP->isBad()) continue;
        cv::Mat cvCorrectedP3Dw(3, 1, CV_32F);
        for (int e = 0; e < 3; ++e) cvCorrectedP3Dw.template at<float>(e) = Xw_out[(size_t)3 * point_index[i] + e];
        pMP->SetWorldPos(cvCorrectedP3Dw);
        pMP->UpdateNormalAndDepth();
    }
}

}  // namespace ORB_SLAM2

#endif

// sim3opt_main.cpp -- drives include/orbslam2_amd/Sim3Optimizer.h on stand-in
// keyframes, MapPoints and a stand-in Sim3 (tests/test_sim3opt.py builds it
// with one g++ line against cvlite.hpp and cvlite_matops.hpp).
//
//   sim3opt_main <scene.bin> <out.txt>
//
// scene.bin, float64 throughout: N1, N2, M, th2, fix_scale, q12[4] (x, y, z,
// w), t12[3], s12, K1[4], K2[4] (fx, fy, cx, cy), T1w[12], T2w[12] (row-major
// [R|t]), mvInvLevelSigma2[8]; N1 rows (x, y, octave, MapPoint of keyframe 1 or
// -1, vpMatches1 entry or -1); N2 rows (x, y, octave); M rows (X, Y, Z, isBad,
// index in keyframe 2 or -1).  out.txt: the return value, the 8 words of g2oS12
// afterwards (hex bit patterns of the doubles q, t, s) and N1 digits: 1 where
// vpMatches1[i] is not NULL.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvlite.hpp"
#include "cvlite_matops.hpp"
#include "orbslam2_amd/Sim3Optimizer.h"

namespace {

struct MiniKeyFrame;

// The members of ORB_SLAM2::MapPoint OptimizeSim3 reads (MapPoint.h:44-62).
struct MiniMapPoint {
    cv::Mat pos = cv::Mat(3, 1, CV_32F);
    bool bad = false;
    int index_in_kf2 = -1;
    const MiniKeyFrame* kf2 = nullptr;
    cv::Mat GetWorldPos() { return pos.clone(); }
    bool isBad() { return bad; }
    int GetIndexInKeyFrame(MiniKeyFrame* pKF) { return pKF == kf2 ? index_in_kf2 : -1; }
};

// ... of ORB_SLAM2::KeyFrame (KeyFrame.h:52-56, :90, :151-165, :186) ...
struct MiniKeyFrame {
    cv::Mat mK = cv::Mat::eye(3, 3, CV_32F);
    cv::Mat Tcw = cv::Mat::eye(4, 4, CV_32F);
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvInvLevelSigma2;
    std::vector<MiniMapPoint*> mvpMapPoints;
    cv::Mat GetRotation() {
        cv::Mat R(3, 3, CV_32F);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R.at<float>(r, c) = Tcw.at<float>(r, c);
        return R;
    }
    cv::Mat GetTranslation() {
        cv::Mat t(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) t.at<float>(r) = Tcw.at<float>(r, 3);
        return t;
    }
    std::vector<MiniMapPoint*> GetMapPointMatches() { return mvpMapPoints; }
};

// ... and of g2o::Sim3 with its two Eigen members (sim3.h:59-62, :280-290).
struct MiniQuat {
    double x_, y_, z_, w_;
    MiniQuat(double w, double x, double y, double z) : x_(x), y_(y), z_(z), w_(w) {}
    double x() const { return x_; }
    double y() const { return y_; }
    double z() const { return z_; }
    double w() const { return w_; }
};
struct MiniVec3 {
    double v[3];
    MiniVec3(double x, double y, double z) : v{x, y, z} {}
    double operator[](int i) const { return v[i]; }
};
struct MiniSim3 {
    MiniQuat r;
    MiniVec3 t;
    double s;
    MiniSim3(const MiniQuat& r_, const MiniVec3& t_, double s_) : r(r_), t(t_), s(s_) {}
    const MiniQuat& rotation() const { return r; }
    const MiniVec3& translation() const { return t; }
    const double& scale() const { return s; }
};

void set_K(cv::Mat& K, const double* k) {
    K.at<float>(0, 0) = (float)k[0], K.at<float>(1, 1) = (float)k[1];
    K.at<float>(0, 2) = (float)k[2], K.at<float>(1, 2) = (float)k[3];
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: sim3opt_main <scene.bin> <out.txt>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<double> buf;
    double v;
    while (std::fread(&v, sizeof(v), 1, f) == 1) buf.push_back(v);
    std::fclose(f);
    const size_t head = 5 + 8 + 8 + 24 + 8;
    if (buf.size() < head) return 2;
    const int N1 = (int)buf[0], N2 = (int)buf[1], M = (int)buf[2];
    const float th2 = (float)buf[3];
    const bool fix_scale = buf[4] != 0.0;
    if (buf.size() != head + (size_t)N1 * 5 + (size_t)N2 * 3 + (size_t)M * 5) return 2;
    MiniSim3 S(MiniQuat(buf[8], buf[5], buf[6], buf[7]), MiniVec3(buf[9], buf[10], buf[11]), buf[12]);
    MiniKeyFrame kf1, kf2;
    set_K(kf1.mK, &buf[13]);
    set_K(kf2.mK, &buf[17]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            kf1.Tcw.at<float>(r, c) = (float)buf[21 + 4 * r + c];
            kf2.Tcw.at<float>(r, c) = (float)buf[33 + 4 * r + c];
        }
    for (int k = 0; k < 8; ++k) {
        kf1.mvInvLevelSigma2.push_back((float)buf[45 + k]);
        kf2.mvInvLevelSigma2.push_back((float)buf[45 + k]);
    }
    const double* rows1 = &buf[head];
    const double* rows2 = rows1 + (size_t)N1 * 5;
    const double* rowsM = rows2 + (size_t)N2 * 3;
    std::vector<MiniMapPoint> points(M);
    for (int m = 0; m < M; ++m) {
        const double* row = rowsM + (size_t)m * 5;
        for (int k = 0; k < 3; ++k) points[m].pos.at<float>(k) = (float)row[k];
        points[m].bad = row[3] != 0.0;
        points[m].index_in_kf2 = (int)row[4];
        points[m].kf2 = &kf2;
    }
    std::vector<MiniMapPoint*> vpMatches1;
    for (int i = 0; i < N1; ++i) {
        const double* row = rows1 + (size_t)i * 5;
        kf1.mvKeysUn.emplace_back((float)row[0], (float)row[1], 31.f, -1.f, 0.f, (int)row[2]);
        kf1.mvpMapPoints.push_back(row[3] >= 0 ? &points[(int)row[3]] : nullptr);
        vpMatches1.push_back(row[4] >= 0 ? &points[(int)row[4]] : nullptr);
    }
    for (int i = 0; i < N2; ++i) {
        const double* row = rows2 + (size_t)i * 3;
        kf2.mvKeysUn.emplace_back((float)row[0], (float)row[1], 31.f, -1.f, 0.f, (int)row[2]);
    }
    int ret;
    try {
        ret = ORB_SLAM2::OptimizeSim3GPU(&kf1, &kf2, vpMatches1, S, th2, fix_scale);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::FILE* o = std::fopen(argv[2], "w");
    if (!o) return 2;
    std::fprintf(o, "%d\n", ret);
    const double out[8] = {S.r.x(), S.r.y(), S.r.z(), S.r.w(), S.t[0], S.t[1], S.t[2], S.s};
    for (int k = 0; k < 8; ++k) {
        uint64_t bits;
        std::memcpy(&bits, &out[k], 8);
        std::fprintf(o, "%016llx ", (unsigned long long)bits);
    }
    std::fprintf(o, "\n");
    for (int i = 0; i < N1; ++i) std::fputc(vpMatches1[i] ? '1' : '0', o);
    std::fprintf(o, "\n");
    std::fclose(o);
    return 0;
}

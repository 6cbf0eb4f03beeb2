// cvlite_matops.hpp -- the two cv::Mat operators Optimizer::OptimizeSim3's
// gather uses (R * P + t on CV_32F matrices), for cvlite.hpp's Mat.  Test
// scaffolding for include/orbslam2_amd/Sim3Optimizer.h only; include it after
// cvlite.hpp and before the adapter header.  The product accumulates in double
// and rounds once to float, the sum is a float addition (OpenCV 2.4's small
// float gemm as recalled; tests/test_sim3opt.py forms its expectation the same
// way).
#ifndef ORBGPU_TESTS_CVLITE_MATOPS_HPP
#define ORBGPU_TESTS_CVLITE_MATOPS_HPP

#include "cvlite.hpp"

namespace cv {

inline Mat operator*(const Mat& a, const Mat& b) {
    Mat m(a.rows, b.cols, CV_32F);
    for (int i = 0; i < a.rows; ++i)
        for (int j = 0; j < b.cols; ++j) {
            double s = 0.0;
            for (int k = 0; k < a.cols; ++k) s += (double)a.at<float>(i, k) * (double)b.at<float>(k, j);
            m.at<float>(i, j) = (float)s;
        }
    return m;
}

inline Mat operator+(const Mat& a, const Mat& b) {
    Mat m(a.rows, a.cols, CV_32F);
    for (int i = 0; i < a.rows; ++i)
        for (int j = 0; j < a.cols; ++j) m.at<float>(i, j) = a.at<float>(i, j) + b.at<float>(i, j);
    return m;
}

}  // namespace cv

#endif
